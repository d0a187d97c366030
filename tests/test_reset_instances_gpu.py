"""GPU tier of test_reset_instances.py: the same scenarios on the shipped HIP library (reset_body of smpc_reset.h as a gfx950 kernel);
the device mask is a torch uint8 tensor."""
import numpy as np
import pytest

import test_reset_instances as T

pytestmark = pytest.mark.gpu


def _torch_mask(m):
    import torch

    t = torch.from_numpy(m).to("cuda")
    torch.cuda.synchronize()
    return t.data_ptr(), t


@pytest.mark.parametrize("kind", T.ALL_KINDS)
def test_cold_start_bitwise(built, kind):
    T.cold_start_bitwise(kind, None)


@pytest.mark.parametrize("kind", T.ALL_KINDS)
def test_isolation_while_walking(built, kind):
    T.isolation_while_walking(kind, None)


@pytest.mark.parametrize("kind", T.ALL_KINDS)
def test_equals_fresh_handle(built, kind):
    T.equals_fresh_handle(kind, None)


@pytest.mark.parametrize("kind", ["go2_kino", "go2_full", "go2_cent"])
def test_recovery_from_a_nan_measurement(built, kind):
    T.recovery(kind, None)


@pytest.mark.parametrize("kind", ["go2_kino", "talos_full", "go2_cent"])
def test_device_mask_equals_host_list(built, kind):
    T.device_mask(kind, None, _torch_mask)


@pytest.mark.parametrize("kind", ["go2_kino", "go2_full", "talos_cent"])
def test_checkpoint_interplay(built, kind):
    T.checkpoint_interplay(kind, None)


@pytest.mark.parametrize("kind", ["go2_kino", "go2_cent"])
def test_retained_derivatives_refuse_until_the_next_iterate(built, kind):
    T.retained_derivatives(kind, None)


def test_device_mask_written_on_the_handles_stream(built):
    """What the mask form is for: the mask is produced on the device, in the handle's own queue (here by torch through
    torch.cuda.ExternalStream), and the reset follows without anything crossing the host."""
    import torch

    kind = "go2_kino"
    B, sub = T.batch_of(kind), T.subset_of(kind)
    a, rb, X = T.make(kind, None)
    b, _, _ = T.make(kind, None)
    a.iterate(X)
    b.iterate(X)
    ext = torch.cuda.ExternalStream(a.stream(), device=torch.device("cuda", 0))
    idx = torch.tensor(sub, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(ext):
        mask = torch.zeros(B, dtype=torch.uint8, device="cuda")
        mask[idx] = 1
    a.reset_instances_device(mask.data_ptr())
    a.wait()
    b.resetInstances(sub)
    T.assert_same(T.snapshot(a), T.snapshot(b), what="after reset")
    assert np.array_equal(mask.cpu().numpy().nonzero()[0], sub)
