"""k_col_full's KEEP (fb_col_full.h): the new stage state of some k3 stays in registers across the four derivative fields instead of
being fetched again.  The same values go through the same operations, so the default build and FB_FULL_KEEP=0 (the KEEP = 0 kernels
of the same library) must agree bit for bit.

Each run is a fresh child process (the switch is read when the context is created).  The state is the parity tests' never-dealiased
noise state (test_gpu_parity._NOISE_CHILD: the Kuo2004 field plus white noise of 1e-4 s^-1), which has energy at every wavenumber, so a
kept k3 that landed in the wrong register could not hide in rounding.  Compared: the vorticity and the whole spectrum (every column,
the frozen ones too) after `steps` steps, and the vorticity after one step more.  No record reads the step's four derivative fields --
every record forms its own from the state (fb_record.h); their reader is the row pass of the next stage, so all of PRIME's and of every
stage's derivative fields up to the last launch of step `steps` enter the vorticity of step `steps + 1`.

Which grids run the kernel: k_col_full needs nx = 4096 or 8192 and a frozen ky = ny/2 column (choose_xpass), which at nx = 4096 means
ny >= 4096.  4096 x 64 and 4096 x 128 therefore take the three-kernel x pass, which the switch does not touch: the cases hold there
trivially and are kept as cheap guards that the switch changes nothing else; 4096^2 (all four stages, PRIME, frozen tiles skipped per
stage) and 8192^2 (NSUB = 2) are the ones that compare KEEP > 0 with KEEP = 0."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

_CHILD = (
    "import hashlib, sys, numpy as np; sys.path[:0]=[%r, %r]\n"
    "import xlab_fftbarotropic_amd as X\n"
    "nx, ny, steps, full = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[5] == '1'\n"
    "rng = np.random.default_rng(29)\n"
    "v0 = rng.standard_normal((nx, ny), dtype=np.float32) * np.float32(1e-4)      # NOT dealiased: energy in every masked mode and in the ky = ny/2 column\n"
    "v0 += X.make_field('kuo2004', nx, ny)\n"
    "m = X.Model(nx, ny, dt=3.0 * 1024 / max(nx, ny)); m.set_vort(v0)\n"
    "res = {}\n"
    "def put(k, t):\n"
    "    a = np.ascontiguousarray(t.cpu().numpy())\n"
    "    res[k] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)\n"
    "    res[k + '_sample'] = a.reshape(-1).view(np.uint32)[::997].copy()\n"
    "    if full: res[k + '_full'] = a\n"
    "m.step(steps); put('vort', m.vort()); put('spec', m.spectrum())\n"
    "m.step(1); put('vort_next', m.vort())\n"
    "np.savez(sys.argv[4], **res)\n"
)

_SWITCHES = ("FB_FULL_KEEP", "FB_FULL_PASS", "FB_FULL_NOSKIP", "FB_NO_COLUMN_SKIP", "FB_NO_ROW8", "FB_NO_ROWH", "FB_ROWQ", "FB_PITCH_EXTRA",
             "FB_PITCH_TUNE", "FB_NO_PITCH_TUNE", "FB_NO_PRESCALE", "FFTBARO_LIB")


def _run(nx, ny, steps, env, tmpdir, tag, full=False):
    e = dict(os.environ)
    for k in _SWITCHES:
        e.pop(k, None)
    e.update(env)
    out = os.path.join(tmpdir, tag + ".npz")
    subprocess.check_call([sys.executable, "-c", _CHILD % (os.path.dirname(HERE), HERE), str(nx), str(ny), str(steps), out, "1" if full else "0"], env=e)
    return np.load(out)


def _assert_same_bits(a, b):
    for k in ("vort", "spec", "vort_next"):
        assert np.array_equal(a[k + "_sample"], b[k + "_sample"]), k
        assert np.array_equal(a[k], b[k]), k                                   # sha256 of the whole field


@pytest.mark.parametrize("nx,ny,steps", [(4096, 64, 3), (4096, 128, 3), (4096, 4096, 3), (8192, 8192, 2)])
def test_keep_is_bitwise_neutral(nx, ny, steps):
    with tempfile.TemporaryDirectory() as d:
        keep = _run(nx, ny, steps, {}, d, "keep")
        keep0 = _run(nx, ny, steps, {"FB_FULL_KEEP": "0"}, d, "keep0")
    _assert_same_bits(keep, keep0)


def test_small_case_matches_the_oracle():
    """4096 x 64 after 3 steps of the noise state against the CPU oracle, to the 1e-5 relative L2 of the other parity tests, in both
    settings of the switch.  (This grid takes the three-kernel x pass, see above; the default path at 4096^2 is held to the oracle on
    the same kind of state by test_gpu_parity.py::test_frozen_mode_shortcuts_are_bitwise_neutral_4096.)"""
    import oracle_py as O
    import ref_numpy as R
    nx, ny, steps = 4096, 64, 3
    with tempfile.TemporaryDirectory() as d:
        keep = _run(nx, ny, steps, {}, d, "keep", full=True)
        keep0 = _run(nx, ny, steps, {"FB_FULL_KEEP": "0"}, d, "keep0", full=True)
    rng = np.random.default_rng(29)
    v0 = rng.standard_normal((nx, ny), dtype=np.float32) * np.float32(1e-4)
    v0 += O.make_field("kuo2004", nx, ny)
    mo = O.Model(nx, ny, dt=3.0 * 1024 / nx)
    mo.set_vort(v0)
    mo.step(steps)
    want = mo.vort()
    for got in (keep, keep0):
        err = R.rel_l2(got["vort_full"], want)
        print("rel L2 against the oracle:", err)
        assert err < 1e-5, err
