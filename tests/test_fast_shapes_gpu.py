"""The one-wave padded chain (csrc/fast_chain.hpp, fast_overlap.hpp) on the device over every class of chain
shape its plan accepts, and the rejected neighbours on the general path (the shape table, the settings and
the well-posed inputs: fast_shapes.py; the same cases on the CPU emulator first: test_fast_shapes_cpu.py).

Tolerances.  Steps: equal bond dimensions and |overlap| within 1e-12 of 1 between the one-wave chain, the
general chain (OCG_NO_FAST=1) and the oracle, <x|dH|x> of the two device results equal to 1e-12
(test_fast_chain.py's).  Overlaps: 1e-12 against the oracle on the padded and on the general contraction
(OCG_NO_FAST_OVL=1).  getHessian at N_t = 7: fused == unfused and hessian_multi == single calls bitwise;
against the oracle gradient 1e-6, Hessian 1e-6 max|H|; against the general chain gradient 1e-12, Hessian
1e-10 max|H|.  Every test prints the deviations it asserts ("FIG ..." lines)."""
import numpy as np
import pytest

import fast_shapes as FS
import oracle_ffi as O

pytestmark = pytest.mark.gpu

N_T = 7


def _engine(monkeypatch, shape, setting=FS.SETTINGS[0], fast=True, fast_ovl=True):
    from optimalcontrolmps_amd.native import Engine
    for name, on in (("OCG_NO_FAST", fast), ("OCG_NO_FAST_OVL", fast_ovl)):
        if on:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, "1")
    maxm, cut = setting
    return Engine(*shape, FS.J, FS.DT, cut, maxm)


def _mps(shape, state):
    from optimalcontrolmps_amd.native import MPS
    return MPS(*shape, *state)


def _orc(m):
    return O.MPS(m.L, m.p, m.Q, m.dims, m.data)


def _fig(shape, what, value):
    print(f"FIG {FS.shape_id(shape)} {what} {value:.3e}")
    return value


@pytest.mark.parametrize("shape", list(FS.ACCEPTED) + list(FS.REJECTED), ids=FS.shape_id)
def test_which_chain_steps(monkeypatch, shape):
    """every accepted shape gets the one-wave chain by default, every rejected neighbour still gets a context"""
    e = _engine(monkeypatch, shape)
    assert e.info.fast_chain == (1 if shape in FS.ACCEPTED else 0)
    e.close()


@pytest.mark.parametrize("setting", FS.SETTINGS, ids=lambda s: "m%d_c%g" % s)
@pytest.mark.parametrize("shape", list(FS.REJECTED), ids=FS.shape_id)
def test_rejected_neighbour_steps(monkeypatch, shape, setting):
    psi, u = _mps(shape, FS.tilted_state(*shape)), FS.controls(*shape)
    st = O.Stepper(*shape, FS.J, FS.DT, setting[1], setting[0])
    e = _engine(monkeypatch, shape, setting)
    assert e.info.fast_chain == 0
    for fwd in (True, False):
        a, ref = e.steps(psi, u, fwd), st.steps(_orc(psi), u, fwd)
        assert list(a.bond_dims()) == list(ref.bond_dims())
        assert _fig(shape, "steps_vs_oracle", abs(abs(st.overlap(ref, _orc(a))) - 1.0)) <= 1e-12
    e.close()


@pytest.mark.parametrize("setting", FS.SETTINGS, ids=lambda s: "m%d_c%g" % s)
@pytest.mark.parametrize("shape", list(FS.ACCEPTED), ids=FS.shape_id)
def test_steps(monkeypatch, shape, setting):
    psi, u = _mps(shape, FS.tilted_state(*shape)), FS.controls(*shape)
    st = O.Stepper(*shape, FS.J, FS.DT, setting[1], setting[0])
    fe, ge = _engine(monkeypatch, shape, setting), _engine(monkeypatch, shape, setting, fast=False)
    assert fe.info.fast_chain == 1 and ge.info.fast_chain == 0
    for fwd in (True, False):
        a, b, ref = fe.steps(psi, u, fwd), ge.steps(psi, u, fwd), st.steps(_orc(psi), u, fwd)
        assert list(a.bond_dims()) == list(b.bond_dims()) == list(ref.bond_dims())
        assert _fig(shape, "steps_vs_oracle", abs(abs(st.overlap(ref, _orc(a))) - 1.0)) <= 1e-12
        assert _fig(shape, "general_steps_vs_oracle", abs(abs(st.overlap(ref, _orc(b))) - 1.0)) <= 1e-12
        assert _fig(shape, "steps_vs_general", abs(abs(fe.overlap(a, b)) - 1.0)) <= 1e-12
        assert _fig(shape, "dH_expectation_vs_general", abs(fe.overlap(a, a, True) - ge.overlap(b, b, True))) <= 1e-12
    fe.close()
    ge.close()


@pytest.mark.parametrize("shape", list(FS.ACCEPTED), ids=FS.shape_id)
def test_overlaps_and_apply_dH(monkeypatch, shape):
    st = O.Stepper(*shape, FS.J, FS.DT, FS.STEPPED[1], FS.STEPPED[0])
    pad = _engine(monkeypatch, shape, FS.STEPPED)
    gen = _engine(monkeypatch, shape, FS.STEPPED, fast_ovl=False)
    assert pad.info.fast_chain == 1 and gen.info.fast_chain == 1
    pairs = FS.overlap_pairs(shape, lambda s, u: (lambda m: (m.dims, m.data))(pad.steps(_mps(shape, s), u, True)))
    for i, (x, y) in enumerate(pairs):
        X, Y = _mps(shape, x), _mps(shape, y)
        ref, ref_dH = st.overlap(_orc(X), _orc(Y)), st.overlap_dH(_orc(X), _orc(Y))
        for name, e in (("padded", pad), ("general", gen)):
            assert _fig(shape, f"{name}_overlap_vs_oracle", abs(e.overlap(X, Y) - ref)) <= 1e-12
            assert _fig(shape, f"{name}_overlap_dH_vs_oracle", abs(e.overlap(X, Y, True) - ref_dH)) <= 1e-12
    # exactApplyMPO runs on the general chain, whose LDS region sits beside the one-wave chain's
    s = _mps(shape, FS.tilted_state(*shape))
    g, nrm = pad.apply_dH(s)
    o = st.apply_dH(_orc(s))
    no = np.sqrt(st.overlap(o, o).real)
    assert _fig(shape, "apply_dH_norm_vs_oracle", abs(nrm - no)) <= 1e-12 * max(1.0, no)
    if shape[1] > 2:  # (hard core: dH = 0, the zero state has no bond dimensions to compare)
        assert list(g.bond_dims()) == list(o.bond_dims())
        assert _fig(shape, "apply_dH_state_vs_oracle", abs(st.overlap(o, _orc(g)).real - no * no) / (no * no)) <= 1e-11
    else:
        assert no == 0.0
    pad.close()
    gen.close()


@pytest.mark.parametrize("shape", list(FS.ACCEPTED), ids=FS.shape_id)
def test_hessian(monkeypatch, shape):
    """getHessian at N_t = 7 with the tilted state as psi_init and the U = 10 ground state as target"""
    ini, tgt = _mps(shape, FS.tilted_state(*shape)), _mps(shape, FS.ground_state(*shape))
    u, u2 = FS.controls(*shape, N_T), FS.controls(*shape, 2 * N_T)[N_T:]
    maxm, cut = FS.SETTINGS[0]
    fe = _engine(monkeypatch, shape)
    assert fe.info.fast_chain == 1
    fe.set_states(tgt, ini)
    Hm, dm, Fm = fe.hessian_multi(np.stack([u, u2]))
    H2, d2, F2 = fe.hessian(u2)
    Hf, df, Ff = fe.hessian(u)
    fe.propagate(u, 3)
    dv, F = fe.div_t(), fe.overlap_factor()
    fe.xi_dH()
    Hu = fe.hessian_rows(u, list(range(1, N_T - 1)), F, dv)
    fe.close()
    assert np.array_equal(Hf, Hu) and np.array_equal(df, dv) and Ff == F  # fused == unfused
    assert np.array_equal(Hm[0], Hf) and np.array_equal(dm[0], df) and Fm[0] == Ff  # K = 2 == two single calls
    assert np.array_equal(Hm[1], H2) and np.array_equal(dm[1], d2) and Fm[1] == F2
    assert shape[1] == 2 or not np.array_equal(Hf, H2)
    oc = O.OC(O.Stepper(*shape, FS.J, FS.DT, cut, maxm), _orc(tgt), _orc(ini), N_T, 0.0)
    Ho, go = oc.hessian(u, 2), oc.gradient(u)
    gf = FS.DT * (df * Ff * 1j).real
    m = np.abs(Ho).max()  # (hard core: dH = 0, the Hessian and the gradient are exact zeros on every path)
    assert (m > 0) == (shape[1] > 2)
    _fig(shape, "hessian_max", m)
    _fig(shape, "gradient_max", np.abs(go).max())
    assert _fig(shape, "gradient_vs_oracle", np.abs(gf - go).max()) <= 1e-6
    assert _fig(shape, "hessian_vs_oracle", np.abs(Hf - Ho).max()) <= 1e-6 * m
    ge = _engine(monkeypatch, shape, fast=False)
    assert ge.info.fast_chain == 0
    ge.set_states(tgt, ini)
    Hg, dg, Fg = ge.hessian(u)
    ge.close()
    gg = FS.DT * (dg * Fg * 1j).real
    assert _fig(shape, "gradient_vs_general", np.abs(gf - gg).max()) <= 1e-12
    assert _fig(shape, "hessian_vs_general", np.abs(Hf - Hg).max()) <= 1e-10 * np.abs(Hg).max()
