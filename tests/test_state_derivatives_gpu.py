"""GPU tier of test_state_derivatives.py: the retained state derivatives of every stage on the shipped HIP library, at the BASELINE
horizons (Go2 H = 50 with the kinodynamics batch of 64; the biped H = 100)."""
import numpy as np
import pytest

import mpc_setup as S
import test_state_derivatives as T

pytestmark = pytest.mark.gpu


def test_go2_kinodynamics_B64_H50():
    T.closed_loop("go2_kino", 64, 13)


def test_talos_fulldynamics_H100():
    T.closed_loop("talos_full", 4, 3, **T.BIPED_DEV)


@pytest.mark.parametrize("family", ["go2_full", "go2_cent"])
def test_go2_families_H50(family):
    T.closed_loop(family, 8, 12)


@pytest.mark.parametrize("family", ["talos_kino", "talos_cent"])
def test_biped_families_H100(family):
    T.closed_loop(family, 4, 3, **T.BIPED_DEV)


@pytest.mark.parametrize("family", ["go2_kino", "go2_full", "go2_cent"])
def test_device_getter_and_checkpoint(family):
    import torch

    make, kw, drive, kind, _, _ = T.FAMILIES[family]
    om, gm, rb = make(4, max_iters=1)
    X = drive(rb, 4, 0, None, om)
    gm.iterate(X)
    with pytest.raises(RuntimeError, match="setRetainStateDerivatives"):
        gm.getStateDerivative(2)
    gm.setRetainStateDerivatives(True)
    with pytest.raises(RuntimeError, match="no iterate"):
        gm.getStateDerivatives()
    Xd = torch.tensor(X, dtype=torch.float64, device="cuda")
    gm.iterate_device(Xd.data_ptr())
    gm.wait()
    xd = gm.getStateDerivatives()
    with pytest.raises(RuntimeError):
        gm.getStateDerivative(gm.H)
    dev = torch.full(xd.shape, float("nan"), dtype=torch.float64, device="cuda")
    gm.get_state_derivatives_device(dev.data_ptr())
    gm.wait()
    assert np.array_equal(dev.cpu().numpy(), xd)
    x01 = np.stack([gm.getStateDerivative(0), gm.getStateDerivative(1)], 1)
    assert S.rel_err(xd[:, :2], x01) <= 1e-12
    blob = gm.save_state()
    gm.load_state(blob)
    with pytest.raises(RuntimeError, match="smpc_load_state"):
        gm.getStateDerivatives()
    gm.iterate(X)
    assert gm.getStateDerivatives().shape == xd.shape
