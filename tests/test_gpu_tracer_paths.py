"""The passive tracer on every kernel path of the engine, against the float64 reference of the coupled system (tests/tracer_numpy.py).

The inputs are tracer_numpy.noisy_inputs: the elliptic vortex and an offset gaussian tracer, each with white noise that was never
dealiased, and a vorticity source.  So both fields carry state in every mode outside the dealiasing circle, where the tracer kernels
have logic of their own (k_tracer_vstate_* and k_advect_deriv pick the base or the stage array per mode, k_beside_update leaves a
masked mode alone and runs on the active column tiles only, ZB is never written at a frozen mode), and the source must reach the
velocity and not the tracer.  tracer_numpy.PATH_CASES holds one row per grid class, with the noise amplitude and step count at which
a reference that is blind to the masked modes of either stage state differs from the true one by >= 1e-4, ten times the parity bar
(asserted on the CPU in tests/test_tracer_cpu.py, stored in the fixture for the slow cases).  One line of figures per case (pytest -s);
DESIGN.md, "Passive tracer", has the table."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import tracer_numpy as T                                        # noqa: E402
from ref_numpy import rel_l2                                    # noqa: E402

SWITCHES = ("FB_FULL_PASS", "FB_FULL_NOSKIP", "FB_NO_COLUMN_SKIP", "FB_NO_ROW8", "FB_ROWQ", "FB_NO_ROWH", "FB_PITCH_EXTRA", "FB_PITCH_TUNE",
            "FB_NO_PITCH_TUNE", "FB_NO_PRESCALE")
CASE_IDS = ["%dx%d" % (k.nx, k.ny) for k in T.PATH_CASES]
GRIDS = [(k.nx, k.ny) for k in T.PATH_CASES]


def _np(t):
    return t.cpu().numpy()


def _case(nx, ny):
    return [k for k in T.PATH_CASES if (k.nx, k.ny) == (nx, ny)][0]


@functools.lru_cache(maxsize=None)
def _inputs(nx, ny, vort_noise):
    out = T.noisy_inputs(nx, ny, vort_noise)
    for a in out:
        a.setflags(write=False)
    return out


def _fixture(case):
    name = "tracer_4096_step%d.npz" % case.steps if case.nx == case.ny == 4096 else "tracer_%dx%d_step%d.npz" % (case.nx, case.ny, case.steps)
    return np.load(os.path.join(HERE, "golden", name))


@functools.lru_cache(maxsize=None)
def _live_reference(nx, ny):
    """(tracer, vort) of the float64 run of a case that is computed here, once"""
    case = _case(nx, ny)
    r = T.recipe_model(nx, ny, *_inputs(nx, ny, case.vort_noise))
    r.step(case.steps)
    out = (r.tracer(), r.vort())
    for a in out:
        a.setflags(write=False)
    return out


def _gpu_model(nx, ny, vort, tracer, source, kappa=T.RECIPE_KAPPA):
    import xlab_fftbarotropic_amd as X
    m = X.Model(nx, ny, nu=T.RECIPE_NU, dt=T.recipe_dt(nx, ny))
    m.set_vort(vort)
    if source is not None:
        m.set_source(source)
    m.set_tracer(tracer, kappa=kappa)
    return m


@pytest.mark.parametrize("case", T.PATH_CASES, ids=CASE_IDS)
def test_path_against_float64(case):
    """set_vort, set_source, set_tracer on the noisy inputs; tracer() at step 0 reproduces the input to 1e-6 (tracer_in, ROW_FWD and
    ROW_INV of this path); after case.steps steps the tracer is within 1e-5 relative L2 of the float64 coupled run and within 4 times
    the vorticity's own error against the same run (the two bars of test_gpu_tracer.py::test_against_float64).  The cases with a
    fixture (16384 x 64, 128 x 16384, 4096^2, 8192^2: the float64 run takes from a minute to several) compare every sub-th point and the
    full-field L2 norms, to 1e-5 as well, rebuild the inputs from the stored seed, and assert the stored probe shifts >= 1e-4."""
    nx, ny = case.nx, case.ny
    if case.fixture:
        G = _fixture(case)
        assert (int(G["seed"]), float(G["vort_noise"]), int(G["steps"])) == (T.RECIPE_SEED, case.vort_noise, case.steps)
        assert (float(G["dt"]), float(G["kappa"]), float(G["nu"])) == (T.recipe_dt(nx, ny), T.RECIPE_KAPPA, T.RECIPE_NU)
        assert float(G["shift_vort"]) >= T.SHIFT_BAR and float(G["shift_tracer"]) >= T.SHIFT_BAR
    v0, c0, src = _inputs(nx, ny, case.vort_noise)
    m = _gpu_model(nx, ny, v0, c0, src)
    e0 = rel_l2(_np(m.tracer()), c0)
    m.step(case.steps)
    gt, gv = m.tracer(), m.vort()
    m.close()
    if case.fixture:
        sx, sy = (int(k) for k in G["sub"])
        et, ev = rel_l2(_np(gt[::sx, ::sy]), G["tracer_sub"]), rel_l2(_np(gv[::sx, ::sy]), G["vort_sub"])
        nt = abs(float(gt.double().pow(2).sum().sqrt()) / float(G["tracer_l2"]) - 1)
        nv = abs(float(gv.double().pow(2).sum().sqrt()) / float(G["vort_l2"]) - 1)
        shifts = (float(G["shift_vort"]), float(G["shift_tracer"]))
    else:
        rt, rv = _live_reference(nx, ny)
        et, ev = rel_l2(_np(gt), rt), rel_l2(_np(gv), rv)
        nt = nv = 0.0
        shifts = (case.shift_vort, case.shift_tracer)
    print("path %dx%d (%s), noise %g, %d steps: tracer rel L2 = %.3g, vorticity rel L2 = %.3g, step 0 %.3g, norms off by %.2g / %.2g; "
          "probe shifts %.3g / %.3g" % (nx, ny, case.what, case.vort_noise, case.steps, et, ev, e0, nt, nv, shifts[0], shifts[1]))
    assert e0 <= 1e-6
    assert et <= 1e-5
    assert et <= 4 * ev
    assert ev <= 1e-5
    assert nt <= 1e-5 and nv <= 1e-5


@pytest.mark.parametrize("nx,ny", GRIDS, ids=["%dx%d" % g for g in GRIDS])
def test_twin_on_every_path(nx, ny):
    """c = zeta with the same noisy state, kappa = nu, no source: rel L2 (tracer, vorticity) <= 1e-5 after the case's steps.
    The two fields go through different kernels, so this catches a wrong stage velocity on every path; it cannot catch a vorticity
    array read in the tracer's place, which is what test_path_against_float64 is for.  Exact zeros are expected on the three-kernel
    path, where the tracer's general transforms and k_col_mid's fused ones round alike; k_col_full (4096^2, 8192^2) rounds differently."""
    noise, steps = _case(nx, ny).vort_noise, _case(nx, ny).steps
    if nx * ny >= 4096 * 4096:
        v0 = T.noisy_vort(nx, ny, noise)
    else:
        v0 = _inputs(nx, ny, noise)[0]
    m = _gpu_model(nx, ny, v0, v0, None, kappa=T.RECIPE_NU)
    assert np.array_equal(_np(m.tracer()).view(np.uint32), _np(m.vort()).view(np.uint32))
    m.step(steps)
    gt, gv = m.tracer(), m.vort()
    moved = rel_l2(_np(gv), v0)
    err = float((gt.double() - gv.double()).pow(2).sum().sqrt() / gv.double().pow(2).sum().sqrt())
    m.close()
    print("twin %dx%d, noise %g, %d steps: rel L2 (tracer, vort) = %.3g; vort moved from its start by %.3g" % (nx, ny, noise, steps, err, moved))
    assert moved > 1e-4
    assert err <= 1e-5


_CHILD = (
    "import sys, numpy as np; sys.path[:0]=[%r, %r, %r]\n"
    "import xlab_fftbarotropic_amd as X, tracer_numpy as T\n"
    "nx, ny, noise, steps, sub = int(sys.argv[1]), int(sys.argv[2]), float(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])\n"
    "v0, c0, src = T.noisy_inputs(nx, ny, noise)\n"
    "m = X.Model(nx, ny, nu=T.RECIPE_NU, dt=T.recipe_dt(nx, ny)); m.set_vort(v0); m.set_source(src); m.set_tracer(c0, kappa=T.RECIPE_KAPPA)\n"
    "m.step(steps)\n"
    "np.savez(sys.argv[6], tracer=m.tracer()[::sub, ::sub].cpu().numpy(), vort=m.vort()[::sub, ::sub].cpu().numpy())\n"
) % (ROOT, HERE, os.path.join(ROOT, "oracle"))


def _child_runs(nx, ny, noise, steps, sub, variants, timeout):
    """the recipe under each set of switches, in child processes (the switches are read when the context is created), one after
    the other"""
    outs = {}
    with tempfile.TemporaryDirectory() as d:
        for tag, extra in variants:
            env = dict(os.environ)
            for k in SWITCHES:
                env.pop(k, None)
            env.update(extra)
            out = os.path.join(d, tag + ".npz")
            subprocess.check_call([sys.executable, "-c", _CHILD, str(nx), str(ny), repr(noise), str(steps), str(sub), out], env=env, timeout=timeout)
            with np.load(out) as z:
                outs[tag] = {k: z[k] for k in z.files}
    return outs


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_row_kernel_switches_4096():
    """64 x 4096: the tracer under k_rowq (default), k_row8 (FB_ROWQ=0) and the Stockham kernel (FB_NO_ROW8=1) agrees within 2e-6, the
    suite's bar for the same maths under another factorisation; the default and FB_ROWQ=0 are not bit-equal, so the switch took"""
    case = _case(64, 4096)
    o = _child_runs(64, 4096, case.vort_noise, case.steps, 1, (("rowq", {}), ("row8", {"FB_ROWQ": "0"}), ("stockham", {"FB_NO_ROW8": "1"})), 120)
    errs = {k: rel_l2(o[k]["tracer"], o["stockham"]["tracer"]) for k in ("rowq", "row8")}
    errs["rowq/row8"] = rel_l2(o["rowq"]["tracer"], o["row8"]["tracer"])
    print("row kernels 64x4096: tracer rel L2 k_rowq / k_row8 against Stockham %.3g / %.3g, k_rowq against k_row8 %.3g" % (errs["rowq"], errs["row8"], errs["rowq/row8"]))
    assert np.isfinite(o["rowq"]["tracer"]).all()
    assert all(e <= 2e-6 for e in errs.values()), errs
    assert not _bits_equal(o["rowq"]["tracer"], o["row8"]["tracer"])
    assert not _bits_equal(o["rowq"]["tracer"], o["stockham"]["tracer"])


def test_row_kernel_switches_8192():
    """64 x 8192: the tracer under k_rowh<1> and under the Stockham kernel (FB_NO_ROWH=1) agrees within 2e-6 and is not bit-equal"""
    case = _case(64, 8192)
    o = _child_runs(64, 8192, case.vort_noise, case.steps, 1, (("rowh", {}), ("stockham", {"FB_NO_ROWH": "1"})), 120)
    err = rel_l2(o["rowh"]["tracer"], o["stockham"]["tracer"])
    print("row kernels 64x8192: tracer rel L2 k_rowh<1> against Stockham %.3g" % err)
    assert np.isfinite(o["rowh"]["tracer"]).all()
    assert err <= 2e-6
    assert not _bits_equal(o["rowh"]["tracer"], o["stockham"]["tracer"])


@pytest.mark.parametrize("n", [4096, 8192])
def test_x_pass_switch(n):
    """n^2, 2 steps of the recipe: the default x pass (k_col_full, the tracer reads its private state layout through
    k_tracer_vstate_full: nsub = 1 at 4096, 2 at 8192) against FB_FULL_PASS=0 (the three column kernels and the tile-major state that
    the strip cases pin to float64): tracer and vorticity within 2e-6, every 4th point, and not bit-equal, so the switch took.
    Both grids are pinned to float64 by their fixtures in test_path_against_float64; this test shows which path that was."""
    o = _child_runs(n, n, 3e-2, 2, 4, (("full", {}), ("three", {"FB_FULL_PASS": "0"})), 300)
    et, ev = rel_l2(o["full"]["tracer"], o["three"]["tracer"]), rel_l2(o["full"]["vort"], o["three"]["vort"])
    print("x pass %d^2, 2 steps: k_col_full against the three-kernel path, tracer rel L2 = %.3g, vorticity rel L2 = %.3g" % (n, et, ev))
    assert np.isfinite(o["full"]["tracer"]).all()
    assert et <= 2e-6 and ev <= 2e-6
    assert not _bits_equal(o["full"]["tracer"], o["three"]["tracer"])
    assert not _bits_equal(o["full"]["vort"], o["three"]["vort"])
