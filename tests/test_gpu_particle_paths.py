"""The Lagrangian particles on every kernel path of the engine, against the float64 reference of the coupled run
(tests/particles_numpy.py: ParticleModel64 on particle_inputs).

The vorticity is the elliptic vortex plus white noise that was never dealiased, with a vorticity source: the flow is unsteady, every
stage state differs from the base, and the modes outside the dealiasing circle carry state.  That is where the particles' stage has
logic of its own: stage_vstate merges base and stage state (k_tracer_vstate_full at nsub 1 and 2, k_tracer_vstate_tm, or ZA/ZB in
place), k_particle_uv_spec picks one of the two per mode, and two fields go through the backward x pass and the path's ROW_INV row
kernel.  particles_numpy.PATH_CASES holds one row per grid class with its bar, in metres of the largest position error: 10 times what
a float32 restatement of the same run on the CPU differs from float64 by.  Two wrong references (the stage array read at a masked
mode; the base read at every stage) miss that bar by a factor of 10 or more on every case: asserted on the CPU in
tests/test_particles_cpu.py, stored in the fixture for the slow cases.  One line of figures per case (pytest -s); DESIGN.md,
"Lagrangian particles", has the table."""
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

import particles_numpy as P                                     # noqa: E402
import tracer_numpy as T                                        # noqa: E402
from ref_numpy import rel_l2                                    # noqa: E402

SWITCHES = ("FB_FULL_PASS", "FB_FULL_NOSKIP", "FB_NO_COLUMN_SKIP", "FB_NO_ROW8", "FB_ROWQ", "FB_NO_ROWH", "FB_PITCH_EXTRA", "FB_PITCH_TUNE",
            "FB_NO_PITCH_TUNE", "FB_NO_PRESCALE")
CASE_IDS = ["%dx%d" % (k.nx, k.ny) for k in P.PATH_CASES]
LX = LY = 600000.0


def _np(t):
    return t.cpu().numpy()


def _same64(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def _bar(case):
    return P.BAR_FACTOR * case.f32


@functools.lru_cache(maxsize=None)
def _inputs(nx, ny, vort_noise):
    out = P.particle_inputs(nx, ny, vort_noise)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _live_reference(nx, ny):
    """(positions, vort) of the float64 run of a case that is computed here, once"""
    case = P.path_case(nx, ny)
    r = P.particle_model(nx, ny, *_inputs(nx, ny, case.vort_noise))
    r.step(case.steps)
    out = (r.particles(), r.vort())
    for a in out:
        a.setflags(write=False)
    return out


def _loaded(cls, nx, ny, vort, source, xy):
    m = cls(nx, ny, nu=T.RECIPE_NU, dt=T.recipe_dt(nx, ny))
    m.set_vort(vort)
    m.set_source(source)
    m.set_particles(xy)
    return m


@pytest.mark.parametrize("case", P.PATH_CASES, ids=CASE_IDS)
def test_path_against_float64(case):
    """set_vort, set_source, set_particles on particle_inputs; particles() straight after returns the input bit for bit; after case.steps
    steps every position is within the case's bar (10 x the float32 restatement's error, from the CPU alone) of the float64 coupled run.
    The live cases also hold the vorticity of the same run to 1e-5 relative L2 of the float64 vorticity; the cases with a fixture
    (16384 x 64, 128 x 16384, 4096^2, 8192^2: the float64 run takes minutes) rebuild the inputs from the stored seed and take the bar and
    the probe shifts from the fixture, which tests/test_particles_cpu.py holds to the case's row."""
    import xlab_fftbarotropic_amd as X
    nx, ny = case.nx, case.ny
    bar, masked, base, moved = _bar(case), case.masked, case.base, case.moved
    if case.fixture:
        G = np.load(os.path.join(HERE, "golden", P.fixture_name(case)))
        assert (int(G["seed"]), float(G["vort_noise"]), int(G["steps"])) == (P.PARTICLE_SEED, case.vort_noise, case.steps)
        assert (float(G["dt"]), float(G["nu"])) == (T.recipe_dt(nx, ny), T.RECIPE_NU)
        bar, masked, base, moved = P.BAR_FACTOR * float(G["f32"]), float(G["shift_masked"]), float(G["shift_base"]), float(G["moved"])
        assert 0.5 <= bar / _bar(case) <= 2.0
        assert min(masked, base) >= P.PROBE_FACTOR * bar and moved >= P.MOVED_FACTOR * bar
    v0, src, x0 = _inputs(nx, ny, case.vort_noise)
    m = _loaded(X.Model, nx, ny, v0, src, x0)
    assert m.particle_count() == P.NPART
    same_in = _same64(_np(m.particles()), x0)
    m.step(case.steps)
    got = _np(m.particles())
    gv = None if case.fixture else _np(m.vort())
    m.close()
    if case.fixture:
        want, ev = G["xy"], 0.0
    else:
        want, rv = _live_reference(nx, ny)
        ev = rel_l2(gv, rv)
    assert want.shape == (P.NPART, 2) and np.isfinite(want).all()
    finite = bool(np.isfinite(got).all())
    err = P.max_shift(got, want) if finite else float("inf")
    print("particle path %dx%d (%s), noise %g, %d steps: max position error %.3g m, bar %.3g m; probe shifts %.3g (masked) / %.3g (base) m, "
          "moved %.3g m (GPU: %.3g m); vorticity rel L2 %.3g" % (nx, ny, case.what, case.vort_noise, case.steps, err, bar, masked, base, moved,
                                                                P.max_shift(got, x0) if finite else float("nan"), ev))
    assert same_in
    assert finite
    assert err <= bar
    assert ev <= 1e-5


_CHILD = (
    "import sys, numpy as np; sys.path[:0]=[%r, %r, %r]\n"
    "import xlab_fftbarotropic_amd as X, particles_numpy as P, tracer_numpy as T\n"
    "nx, ny, noise, steps = int(sys.argv[1]), int(sys.argv[2]), float(sys.argv[3]), int(sys.argv[4])\n"
    "v0, src, x0 = P.particle_inputs(nx, ny, noise)\n"
    "m = X.Model(nx, ny, nu=T.RECIPE_NU, dt=T.recipe_dt(nx, ny)); m.set_vort(v0); m.set_source(src); m.set_particles(x0)\n"
    "m.step(steps)\n"
    "np.savez(sys.argv[5], xy=m.particles().cpu().numpy(), x0=x0)\n"
) % (ROOT, HERE, os.path.join(ROOT, "oracle"))


def _child_runs(nx, ny, noise, steps, variants, timeout):
    """the positions of the case's inputs after `steps` steps under each set of switches, in child processes (the switches are read when
    the context is created), one after the other"""
    outs = {}
    with tempfile.TemporaryDirectory() as d:
        for tag, extra in variants:
            env = dict(os.environ)
            for k in SWITCHES:
                env.pop(k, None)
            env.update(extra)
            out = os.path.join(d, tag + ".npz")
            subprocess.check_call([sys.executable, "-c", _CHILD, str(nx), str(ny), repr(noise), str(steps), out], env=env, timeout=timeout)
            with np.load(out) as z:
                outs[tag] = z["xy"]
                assert np.isfinite(outs[tag]).all() and not _same64(outs[tag], z["x0"]), tag
    return outs


def _check_pairs(label, o, bar, pairs):
    errs = {"%s/%s" % ab: P.max_shift(o[ab[0]], o[ab[1]]) for ab in pairs}
    print("%s: positions differ by %s m; bar %.3g m" % (label, ", ".join("%s %.3g" % kv for kv in errs.items()), bar))
    for (a, b), e in zip(pairs, errs.values()):
        assert e <= bar, (a, b, e, bar)
        assert not _same64(o[a], o[b]), (a, b)


@pytest.mark.parametrize("n", [4096, 8192])
def test_x_pass_switch(n):
    """n^2, 2 steps of the case's inputs: the default x pass (k_col_full; the particles read its private state layout through
    k_tracer_vstate_full, nsub = 1 at 4096 and 2 at 8192) against FB_FULL_PASS=0 (the three column kernels and the tile-major state that
    the strip cases pin to float64): positions within the case's bar and not bit-equal, so the switch took.  Both grids are pinned to
    float64 in test_path_against_float64; this test shows which path that was."""
    case = P.path_case(n, n)
    o = _child_runs(n, n, case.vort_noise, 2, (("full", {}), ("three", {"FB_FULL_PASS": "0"})), 300)
    _check_pairs("x pass %d^2, 2 steps, k_col_full against the three-kernel path" % n, o, _bar(case), [("full", "three")])


def test_row_kernel_switches():
    """64 x 4096: the positions under k_rowq (default), k_row8 (FB_ROWQ=0) and the Stockham kernel (FB_NO_ROW8=1); 64 x 8192: under
    k_rowh<1> (default) and the Stockham kernel (FB_NO_ROWH=1).  Every pair within the case's bar and not bit-equal, so the switch took."""
    case = P.path_case(64, 4096)
    o = _child_runs(64, 4096, case.vort_noise, case.steps, (("rowq", {}), ("row8", {"FB_ROWQ": "0"}), ("stockham", {"FB_NO_ROW8": "1"})), 120)
    _check_pairs("row kernels 64x4096", o, _bar(case), [("rowq", "row8"), ("rowq", "stockham"), ("row8", "stockham")])
    case = P.path_case(64, 8192)
    o = _child_runs(64, 8192, case.vort_noise, case.steps, (("rowh", {}), ("stockham", {"FB_NO_ROWH": "1"})), 120)
    _check_pairs("row kernels 64x8192", o, _bar(case), [("rowh", "stockham")])


@pytest.mark.parametrize("nx,ny", [(64, 16384), (16384, 64)])
def test_sample_on_long_axes(nx, ny):
    """Model.sample against lagrange4_sample on the same random float32 field where one axis has 16384 points: 1000 positions that
    include grid points, the first and the last cell of the long axis and positions 3 domain lengths away, within 1e-12 max|field|
    (both sides are float64 arithmetic on identical data); on grid points the float32 value itself, widened."""
    import xlab_fftbarotropic_amd as X
    m = X.Model(nx, ny, LX, LY)
    rng = np.random.default_rng(13)
    f = rng.standard_normal((nx, ny)).astype(np.float32)
    xy = P.seed_positions(nx, ny, LX, LY, P.NPART, seed=17)
    dx, dy = P.widen(LX) / nx, P.widen(LY) / ny
    cell = np.floor(xy / np.array([dx, dy])).astype(np.int64)
    long_axis = 0 if nx > ny else 1
    n_long = max(nx, ny)
    assert (cell[:, long_axis] == n_long - 1).any() and (cell[:, long_axis] == 0).any()         # first and last cell of the long axis
    assert (np.abs(xy[:, long_axis]) > 2.5 * LX).any()                                          # and far positions
    want = P.lagrange4_sample(f, xy, LX, LY)
    got = _np(m.sample(f, xy))
    err, scale = P.max_shift(got, want), float(np.max(np.abs(f)))
    g = P.grid_points(nx, ny, LX, LY, 64)
    i = np.mod(np.round(g[:, 0] / dx).astype(np.int64), nx)
    j = np.mod(np.round(g[:, 1] / dy).astype(np.int64), ny)
    on_grid = _np(m.sample(f, g))
    m.close()
    print("sample %dx%d: max err %.3e, max|f| %.3e, %d grid points" % (nx, ny, err, scale, g.shape[0]))
    assert got.shape == (P.NPART,)
    assert err <= 1e-12 * scale
    assert g.shape[0] >= 32
    assert (i == nx - 1).any() and (j == ny - 1).any()                                          # the far corner is among them
    assert _same64(on_grid, f[i, j].astype(np.float64))


def test_slab_of_one_rank_on_tile_major_state():
    """1024 x 64: EngineSlab of one rank (always the three-kernel x pass, here with tile-major state: k_tracer_vstate_tm through the
    slab's entry points) gives the positions of Model after the case's steps bit for bit, on the case's unsteady inputs"""
    import xlab_fftbarotropic_amd as X
    from importlib import import_module
    S = import_module("xlab-fftbarotropic_amd.slab")
    case = P.path_case(1024, 64)
    v0, src, x0 = _inputs(1024, 64, case.vort_noise)
    outs = []
    for cls in (X.Model, S.EngineSlab):
        m = _loaded(cls, 1024, 64, v0, src, x0)
        m.step(case.steps)
        outs.append(_np(m.particles()))
        m.close()
    assert np.isfinite(outs[0]).all() and not _same64(outs[0], x0)
    assert _same64(outs[1], outs[0])
