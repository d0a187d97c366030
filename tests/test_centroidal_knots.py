"""The LQ knots of the centroidal engines against the oracle's, and the debug read-outs that carry them.

Knot parity: every field of every stage of debug_lq (point feet: the stage record of the kernel pipeline, unpacked through CentRec's own maps;
6-D feet: the dense knot of riccati_dense_body<Cent6Dims>) against the oracle's knot of the same iteration, the terminal node against the
oracle's, preg against the oracle's regularisation of that iteration.  The norm is per stage and per field, max|a - b| / max|b|, not floored; a
block the oracle holds at exactly zero must be exactly zero.  Bars: 1e-9 on the emulated bodies (the emulation tier's own); on the device 1e-8
for the matrices, f and d, 1e-6 for the Lagrangian gradients q, r and qN (the bars of test_gpu_parity.py::test_stage_knots_match_oracle).

The residual vectors need more than their bar in that norm, and why: f, d, q, r and qN are DIFFERENCES that cancel -- f = (x (+) dt xdot) -
x+ + mu (lam_e - lam) is 1e-7 .. 1e-9 of |x+| near a solution, and likewise d against the cone value, q, r, qN against the multiplier terms --
so relative to their own size a rounding of the terms (eps |x+| / |f|) or the 1e-10 distance of the two iterates shows as 1e-9 .. 1e-3
and more (observed on the emulated bodies: f 3.8e-9 in cent_record_k1 and O(1) in cent_h65, where f is rounding alone; r 2.3e-4, qN 3.3e-4 in
cent_record_k3; every run prints the worst raw figure of each).  They are therefore gated against the terms they are differences of,
max|a - b| / max(max|b|, scale) with scale = max|x_{t+1}| for f, max|D u_t| for d, max(|lam_t|, |lam_{t+1}|, |C^T nu_t|, |Q x_t|) for q,
max(|B^T lam_{t+1}|, |D^T nu_t|, |R u_t|) for r and max|lam_H| for qN (the oracle's), at the same bars; the matrices stay unfloored.
Observed against the bars: emulated bodies matrices <= 1.7e-11, residual vectors <= 1e-9; MI355X matrices <= 1.1e-11, residual vectors <= 1e-9 --
r of talos_cent_tight 9.9e-10 on both (the multipliers of product and oracle differ by 6e-9 there: a rounding of the cone value amplified by
1 / mu, which D^T carries into r).

The steps: debug_steps / debug_dual_steps of the pipeline read the ring slots the kernels write (x_after = x_before + alpha dx for every stage)."""
import numpy as np
import pytest

import mpc_setup as S
import oracle_lib as O
import sweep_check as SC
import test_sweeps as T

PARITY = ["cent_record_k1", "cent_record_k3", "cent_cones_backtrack", "cent_h65", "talos_cent_walk", "talos_cent_tight"]
MATS = ("A", "B", "Q", "S", "R", "D", "f", "d")
GRADS = ("q", "r")


def _gap(a, b, what, scale=0.0):
    den = np.abs(b).max()
    if den == 0.0:
        assert np.all(a == 0.0), (what, "the oracle's block is exactly zero, the product's is not", float(np.abs(a).max()))
        return 0.0
    return float(np.abs(a - b).max() / max(den, scale))


def _scales(om, ko, b, t):
    """Size of the terms the residual vectors of stage t are differences of (module docstring), from the oracle's iterate and knot."""
    xs, us, lams, vs = om_cache(om)
    return dict(f=np.abs(xs[b, t + 1]).max(), d=np.abs(ko["D"] @ us[b, t]).max(),
                q=max(np.abs(lams[b, t]).max(), np.abs(lams[b, t + 1]).max(), np.abs(ko["C"].T @ vs[b, t]).max(), np.abs(ko["Q"] @ xs[b, t]).max()),
                r=max(np.abs(ko["B"].T @ lams[b, t + 1]).max(), np.abs(ko["D"].T @ vs[b, t]).max(), np.abs(ko["R"] @ us[b, t]).max()))


_cache = {}


def om_cache(om):
    key = id(om)
    if _cache.get("key") != key or _cache.get("stamp") != om_stamp(om):
        _cache.update(key=key, stamp=om_stamp(om), val=(om.xs, om.us, om.lams, om.vs))
    return _cache["val"]


def om_stamp(om):
    return float(om.info[0, 0])


def _assert_pad_decoupled(kg, QNp, qNp, what):
    """6-D feet: the state of the dense sweep is padded from 9 to 12.  The three pad rows and columns of every block must be exactly zero --
    no entry couples a pad state to a real one, to a control, to a cone row or to the cost -- so that the sweep on 12 is the sweep on 9."""
    for k, v in kg["pad"].items():
        assert not np.any(v), (what, "pad block %s of the 6-D knot is not exactly zero" % k)
    assert not np.any(QNp[9:, :]) and not np.any(QNp[:, 9:]) and not np.any(qNp[9:]), (what, "pad block of the terminal node")


def _knot_parity(name, lib, bar_mat, bar_grad):
    """THE test that catches a wrong CentRec::m2_off / ab_off: the accessor unpacks the record through the very maps cent_bwd_body gathers its
    KKT matrix through, so a map that sends an entry to the wrong place sends it to the wrong place here too, and the oracle's knot disagrees.
    (The sweep check of test_sweeps.py cannot see that: there both sides read through the same maps.)"""
    worst, raw = {}, {}
    for label, gm, om in T.CENT_SCENARIOS[name](lib, paired=True):
        cent6 = SC.kind_of(gm) == "cent6"
        for b in range(gm.B):
            for t in range(gm.H):
                kg, ko = gm.debug_lq(b, t), om.knot(b, t)
                what = (name, label, "instance %d" % b, "stage %d" % t)
                dev = dict(kg, D=kg["Dd"])
                if cent6:
                    g = _gap(kg["Cd"], ko["C"], what + ("C",))
                    worst["C"] = max(worst.get("C", 0.0), g)
                    assert g < bar_mat, what + ("C", g, bar_mat)
                else:
                    assert not ko["C"].any(), what + ("the oracle's C is structurally zero for point feet",)
                    assert kg["any"] == float(kg["act"].any()), what + ("any",)
                # which rows are present: the oracle zeroes the rows of [C D] that are not active
                assert np.array_equal(kg["act"] != 0.0, (np.abs(ko["D"]).sum(1) + np.abs(ko["C"]).sum(1)) != 0.0), what + ("activity",)
                sc = _scales(om, ko, b, t)
                for k in MATS + GRADS:
                    g = _gap(dev[k], ko[k], what + (k,), sc.get(k, 0.0))
                    worst[k] = max(worst.get(k, 0.0), g)
                    if k in sc:
                        raw[k] = max(raw.get(k, 0.0), _gap(dev[k], ko[k], what + (k,)))
                    bar = bar_grad if k in GRADS else bar_mat
                    assert g < bar, what + (k, g, bar)
            oQ, oq, opreg = om.terminal_knot(b)
            QN, qN = gm.debug_terminal(b)
            what = (name, label, "instance %d" % b, "terminal node")
            lamH = np.abs(om_cache(om)[2][b, -1]).max()
            raw["qN"] = max(raw.get("qN", 0.0), _gap(qN, oq, what + ("qN",)))
            for k, a, r, bar in (("QN", QN, oQ, bar_mat), ("qN", qN, oq, bar_grad)):
                g = _gap(a, r, what + (k,), lamH if k == "qN" else 0.0)
                worst[k] = max(worst.get(k, 0.0), g)
                assert g < bar, what + (k, g, bar)
            if cent6:
                QNp, qNp = gm.debug_terminal(b, padded=True)
                for t in range(gm.H):
                    _assert_pad_decoupled(gm.debug_lq(b, t), QNp, qNp, (name, label, b, t))
                # (no scalar read-out of preg on this path: it is on the diagonal of R, compared above, and of QN)
            else:
                preg = gm.debug_lq(b, 0)["preg"]
                assert abs(preg - opreg) <= 1e-15 * opreg, what + ("preg", preg, opreg)
    e = lambda d: " ".join("%s %.1e" % kv for kv in sorted(d.items()))
    print("knot parity %s: worst per-stage, per-field gap %s | bars %.0e (q, r, qN: %.0e) | residual vectors relative to their own size (not "
          "gated) %s" % (name, e(worst), bar_mat, bar_grad, e(raw)))


@pytest.mark.parametrize("name", PARITY)
def test_emulated_knots_match_oracle(built, name):
    _knot_parity(name, S.emu_lib(), 1e-9, 1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_hip_knots_match_oracle(built, name):
    _knot_parity(name, None, 1e-8, 1e-6)


# ---- debug_steps / debug_dual_steps of the pipeline: the ring ----
def _steps_on_the_ring(lib):
    """x_after = x_before + alpha dx for ALL stages of both instances after 3 control steps (ring head 3), with the iterate before the step
    rebuilt from the previous control step's outputs: a max_iters = 1 handle shifts its warm start by one stage (stage H repeats stage H - 1),
    and stage 0 is the measured state.  The same for us, vs and lams with debug_dual_steps.  The parent's debug_steps read buf.dxs / buf.dus
    linearly: rotated stages, and for dus stride H instead of H + 1 -- this test fails on it."""
    gm, _, rb = T._go2_cent(lib, 2, 1)
    X = S.random_states(rb, 2)
    X = T._cent_steps(gm, None, rb, X, 2)
    xs0, us0, vs0, lams0 = gm.xs.copy(), gm.us.copy(), gm.vs.copy(), gm.lams.copy()
    gm.iterate(X)
    alpha = gm.info[:, 2][:, None, None]
    dxs, dus = gm.debug_steps()
    dvs, dlams = gm.debug_dual_steps()
    assert np.all(dxs[:, 0] == 0.0) and np.all(dlams[:, 0] == 0.0)
    # warm start: x_t <- x_{t+1} (t < H), x_H <- x_H ; u, v, lam_{t+1} likewise with a fresh last stage (u: the repeat, v and lam: zero)
    xb = np.concatenate([xs0[:, 1:], xs0[:, -1:]], 1)
    ub = np.concatenate([us0[:, 1:], us0[:, -1:]], 1)
    vb = np.concatenate([vs0[:, 1:], np.zeros_like(vs0[:, -1:])], 1)
    lb = np.concatenate([lams0[:, :1], lams0[:, 2:], np.zeros_like(lams0[:, -1:])], 1)
    tol = 1e-12  # (an addition of FP64 numbers of the size of the iterate, compared relative to it)
    for name, after, before, step in (("xs", gm.xs[:, 1:], xb[:, 1:], dxs[:, 1:]), ("us", gm.us, ub, dus), ("vs", gm.vs, vb, dvs),
                                      ("lams", gm.lams[:, 1:], lb[:, 1:], dlams[:, 1:])):
        for t in range(after.shape[1]):
            want = before[:, t] + alpha[:, 0] * step[:, t]
            err = np.abs(after[:, t] - want).max() / max(np.abs(after[:, t]).max(), 1e-300)
            assert err < tol, (name, "stage %d" % t, err)
    assert np.abs(dus).max() > 0 and np.abs(dxs).max() > 0


def test_emulated_debug_steps_follow_the_ring(built):
    _steps_on_the_ring(S.emu_lib())


@pytest.mark.gpu
def test_hip_debug_steps_follow_the_ring(built):
    _steps_on_the_ring(None)


# ---- accessor errors ----
def _accessor_errors(lib):
    gm, _, rb = T._go2_cent(lib, 2, 1, horizon=5)
    gm.iterate(S.random_states(rb, 2))
    gm.debug_lq(1, 4)
    for inst, t in ((2, 0), (-1, 0), (0, 5), (0, -1)):
        with pytest.raises(RuntimeError, match="Stage index exceeds stage vector size"):
            gm.debug_lq(inst, t)
    for inst in (2, -1):
        with pytest.raises(RuntimeError, match="instance index out of range"):
            gm.debug_terminal(inst)
    # a kinodynamics handle has no multiplier-step read-out
    gk, _, _, _ = S.make_product(1, lib=lib, horizon=5)
    with pytest.raises(RuntimeError, match="smpc_debug_get_dual_steps needs a centroidal handle"):
        gk.debug_dual_steps()


def test_emulated_accessor_errors(built):
    _accessor_errors(S.emu_lib())


@pytest.mark.gpu
def test_hip_accessor_errors(built):
    _accessor_errors(None)


def _fused_handle_refuses(lib):
    """A handle of the one-kernel form (SMPC_CENT_FUSED=1 of a cross-check build) has no record: the knot read-outs answer INVALID and say
    why -- they must not return zeros; its steps stay linear in t."""
    gm, _, rb = T._go2_cent(lib, 2, 1, horizon=5, env={"SMPC_CENT_FUSED": "1"})
    gm.iterate(S.random_states(rb, 2))
    for call in (lambda: gm.debug_lq(0, 0), lambda: gm.debug_terminal(0)):
        with pytest.raises(RuntimeError, match="SMPC_CENT_FUSED=1 runs the one-kernel control step, which keeps no stage record"):
            call()
    dxs, dus = gm.debug_steps()
    ref, _, _ = T._go2_cent(lib, 2, 1, horizon=5)
    ref.iterate(S.random_states(rb, 2))
    rx, ru = ref.debug_steps()
    assert np.abs(dxs).max() > 0 and S.rel_err(rx, dxs) < 1e-9 and S.rel_err(ru, dus) < 1e-8


def test_emulated_fused_handle_has_no_knots(built):
    _fused_handle_refuses(S.emu_lib())


@pytest.mark.gpu
def test_hip_fused_handle_has_no_knots(built):
    _fused_handle_refuses(S.xcheck_lib())
