"""The entry layer of the C ABI on the GPU (csrc/fb_entry.h): every fb_model_X / fb_slab_X[_local] pair is one body behind one guard
layer.  Two checks at 64 x 64.

The refusal table, tests/golden/entry_refusals.json, was recorded twice (tests/golden/make_entry_fixture.py): from the hand-written
pairs at 321421f, and again at e2fbb09 with the five pairs of the tangent subspace added, every earlier entry unchanged.  It holds
every paired function before its feature is set, on a slab of two ranks where it supports one, on a slab that is not connected, and
with each numeric argument out of its range.  Every entry has one thing wrong and is refused before anything is launched.  Asserted:
the status and the telling phrase of the recording, and that the message starts with the function's own name.

The pairs: from the same state, after 3 steps with a tracer, a tangent, 100 particles and an adjoint variable, every getter of Model and
of an EngineSlab of one rank returns the same bits.  One output cannot: the mean columns of the azimuthal table are sums of global
float64 atomics, which "arrive in whatever order the atomics land" (csrc/fb_azim.h), so two calls on one Model differ in the last bits
too.  Its bin edges, counts and centre are compared bit for bit, and its mean columns are held, for both handles, to the bound of
tests/test_gpu_azimuthal.py against the float64 table of the (bit-identical) fields: 1e-9 <|term|>, the float64 summation bound."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import azimuthal_numpy as A                                     # noqa: E402
import entry_cases as E                                         # noqa: E402
import tangent_numpy as G                                       # noqa: E402


def test_refusals_are_those_of_the_hand_written_pairs():
    table = json.load(open(os.path.join(HERE, "golden", "entry_refusals.json")))
    assert [(e["fn"], e["args"], e["phrase"]) for e in table] == [(fn, args, phrase) for fn, args, phrase in E.ENTRIES]
    paired = {"fb_model_" + n for n in PAIRED} | {"fb_slab_" + n for n in PAIRED} | {"fb_slab_" + n + "_local" for n in PAIRED}
    assert {e["fn"] for e in table} <= paired
    h = E.Handles()
    bad = []
    try:
        for e in table:
            rc, msg = h.call(e["fn"], e["args"])
            print("%-40s %-50s -> %d %s" % (e["fn"], json.dumps(e["args"]), rc, msg if rc else ""))
            if rc != e["rc"] or (rc and not (e["phrase"] in msg and msg.startswith(e["fn"] + ": "))):
                bad.append((e["fn"], e["args"], e["rc"], e["phrase"], rc, msg))
    finally:
        h.close()
    assert not bad, bad


# the paired functions (binding.SIGNATURES) that the table has a refusal of
PAIRED = ("set_vort", "step", "time_steps", "get_vort", "get_diag", "get_okubo_weiss", "get_eddy_diffusivity", "get_pressure", "get_spectra",
          "get_azimuthal", "set_tracer", "get_tracer", "get_tracer_eddy_diffusivity", "set_particles", "get_particles", "sample",
          "set_tangent", "get_tangent", "tangent_norm", "tangent_scale", "set_tangents", "get_tangents", "tangent_count", "tangent_gram",
          "tangent_qr", "adjoint_record", "adjoint_recorded", "set_adjoint", "get_adjoint",
          "adjoint_back")


def test_every_paired_function_has_a_refusal_in_the_table():
    """all of binding._PAIRS but destroy (NULL is fine), set_source (no refusal but the NULL handle) and particle_count (likewise)"""
    import xlab_fftbarotropic_amd as X
    B = sys.modules[X.Model.__module__]
    names = {n.replace("_local", "") for n in B._PAIRS} - {"destroy", "set_source", "particle_count"}
    assert names == set(PAIRED)
    seen = {fn.replace("fb_model_", "").replace("fb_slab_", "").replace("_local", "") for fn, _, phrase in E.ENTRIES if phrase}
    assert seen == set(PAIRED)


L = 600000.0


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy())
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _outputs(m, v0, d0, c0, x0, steps):
    """every paired getter of m after `steps` steps from v0 with a tracer, a tangent, particles and the adjoint's tape; {name: bits}"""
    m.set_vort(v0)
    m.set_tracer(c0, kappa=2.0)
    m.set_tangent(d0)
    m.set_particles(x0)
    m.record_adjoint(steps)
    m.step(steps)
    out = {"recorded": m.adjoint_recorded(), "count": m.particle_count(), "norm": np.float64(m.tangent_norm("energy")).view(np.uint64)}
    vort = m.vort()
    out["vort"] = _bits(vort)
    for name, f in zip(("psi", "u", "v"), m.diag()):
        out[name] = _bits(f)
    for name, f in zip(("W", "tau"), m.okubo_weiss()):
        out[name] = _bits(f)
    for name, f in zip(("keff", "keff_zeta", "keff_grad2"), m.eddy_diffusivity(32, fields=True)):
        out[name] = _bits(f)
    out["pressure"] = _bits(m.pressure(ref=(3, 5)))
    out["spectra"] = _bits(m.spectra())
    nbins, dr = A.default_bins(E.N, E.N, L, L)
    table, center = m.azimuthal("psi-min", nbins=nbins, dr=dr, nmodes=2)
    out["azimuthal_bins"], out["center"], out["_azimuthal"] = _bits(table[:, :3].contiguous()), _bits(center), table.cpu().numpy()
    out["tracer"] = _bits(m.tracer())
    for name, f in zip(("tracer_keff", "tracer_c", "tracer_grad2"), m.tracer_eddy_diffusivity(32, fields=True)):
        out[name] = _bits(f)
    out["particles"] = _bits(m.particles())
    out["sample"] = _bits(m.sample(vort))
    out["tangent"] = _bits(m.tangent())
    m.set_adjoint(vort)
    m.adjoint_back(steps)
    out["adjoint"] = _bits(m.adjoint())
    out["recorded_after"] = m.adjoint_recorded()
    m.record_adjoint(0)
    m.close()
    return out


def test_model_and_slab_of_one_rank_return_the_same_bits():
    import xlab_fftbarotropic_amd as X
    from importlib import import_module
    S = import_module("xlab-fftbarotropic_amd.slab")
    n, steps = E.N, 3
    v0, d0, _ = G.tangent_inputs(n, n, G.PATH_CASES[0].vort_noise)
    c0 = np.roll(v0, 11, axis=1).copy()
    x0 = np.random.default_rng(7).uniform(0.0, 6.0e5, (100, 2))
    a = _outputs(X.Model(n, n, nu=G.NU, dt=3.0), v0, d0, c0, x0, steps)
    b = _outputs(S.EngineSlab(n, n, nu=G.NU, dt=3.0), v0, d0, c0, x0, steps)
    assert a["recorded"] == steps and a["recorded_after"] == 0 and a["count"] == 100
    assert sorted(a) == sorted(b)
    differ = [k for k in a if not k.startswith("_") and not np.array_equal(a[k], b[k])]
    assert not differ, differ
    zeta, u, v = (a[k].view(np.float32) for k in ("vort", "u", "v"))
    xc, yc = a["center"].view(np.float64)[:2]
    nbins, dr = A.default_bins(n, n, L, L)
    want, scale = A.table(zeta, u, v, L, L, xc, yc, nbins, dr, 2)
    for who, got in (("model", a["_azimuthal"]), ("slab", b["_azimuthal"])):
        worst = float(np.max(np.abs(got - want)[:, 3:] - 1e-9 * scale[:, 3:]))
        print("azimuthal means, %s: largest error minus its bound %.3g" % (who, worst))
        assert worst <= 0.0, who
    for k in ("vort", "tracer", "tangent", "adjoint", "pressure", "particles"):
        assert a[k].any(), k                                    # (not the bits of zeros)
