#!/usr/bin/env python3
"""Bitwise comparison of two library builds on a noisy 4096^2 (or given) state:
tools/cmp_variants.py <alt.so|-> [n=4096] [steps=3] [--records] [KEY=VAL ...]
Runs each build in its own process (FFTBARO_LIB; "-" = the in-tree library both times) and compares vort / spectrum bit for bit; with
--records also diag (psi, u, v), okubo_weiss (W, tau), pressure (pres, reference point (3, 5); only when both builds export
fb_model_get_pressure) and eddy_diffusivity (zeta, grad2 and the table), where columns 5-8 of the table
are f64 sums in the order of LDS atomics and are compared to rounding (relative 1e-9).  Whole fields are compared by sha256, so 16384^2
fits.  KEY=VAL pairs are set in the environment of the second run only (run-time switches)."""
import os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import hashlib, sys, numpy as np
sys.path.insert(0, %r)
import xlab_fftbarotropic_amd as X
n, steps, records = int(sys.argv[1]), int(sys.argv[2]), sys.argv[4] == "1"
rng = np.random.default_rng(5)
v0 = (rng.standard_normal((n, n)) * 1e-4).astype(np.float32) + X.make_field("kuo2004", n)
m = X.Model(n, n, dt=3.0 * 1024 / n)
m.set_vort(v0)
m.step(steps)
out, res = {"vort": m.vort(), "spec": m.spectrum()}, {}
if records:
    out["psi"], out["u"], out["v"] = m.diag()
    out["W"], out["tau"] = m.okubo_weiss()
    table, out["zeta"], out["grad2"] = m.eddy_diffusivity(fields=True)
    res["table"] = table.cpu().numpy()
    if hasattr(X.lib(), "fb_model_get_pressure"):
        out["pres"] = m.pressure(ref=(3, 5))
for k, t in out.items():
    a = np.ascontiguousarray(t.cpu().numpy())
    res[k] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
    res[k + "_sample"] = a.reshape(-1)[::997].copy()                     # for the size of a difference
np.savez(sys.argv[3], **res)
''' % ROOT
records = "--records" in sys.argv
argv = [a for a in sys.argv if a != "--records"]
alt = None if argv[1] == "-" else os.path.abspath(argv[1]); n = int(argv[2]) if len(argv) > 2 else 4096; steps = int(argv[3]) if len(argv) > 3 else 3
extra = dict(a.split("=", 1) for a in argv[4:])
with tempfile.TemporaryDirectory() as d:
    outs = []
    for tag, lib in (("base", None), ("alt", alt)):
        e = dict(os.environ)
        e.pop("FFTBARO_LIB", None)
        if lib:
            e["FFTBARO_LIB"] = lib
        if tag == "alt":
            e.update(extra)
        o = os.path.join(d, tag + ".npz")
        subprocess.check_call([sys.executable, "-c", CHILD, str(n), str(steps), o, "1" if records else "0"], env=e)
        outs.append(np.load(o))
    has_pres = records and all("pres" in o.files for o in outs)
    if records and not has_pres:
        print("pres not compared: a build does not export fb_model_get_pressure")
    for k in ("vort", "spec") + (("psi", "u", "v", "W", "tau", "zeta", "grad2") if records else ()) + (("pres",) if has_pres else ()):
        same = np.array_equal(outs[0][k], outs[1][k])
        a, b = outs[0][k + "_sample"], outs[1][k + "_sample"]
        print(k, "bitwise equal" if same else "DIFFERENT: max abs diff on a sample %g" % np.abs(a - b).max())
    if records:
        a, b = outs[0]["table"], outs[1]["table"]
        exact = np.array_equal(a[:, :5].view(np.uint64), b[:, :5].view(np.uint64))
        rel = (np.abs(a[:, 5:] - b[:, 5:]) / np.maximum(np.abs(a[:, 5:]), 1e-300)).max()
        print("keff table", "columns 0-4 bitwise equal" if exact else "columns 0-4 DIFFERENT", "| columns 5-8 max rel diff %.2e" % rel,
              "(within rounding)" if rel <= 1e-9 else "(BEYOND 1e-9)")
