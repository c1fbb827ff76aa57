#!/usr/bin/env python3
"""The bits of the tangent's norm and of the Gram matrix (tests/test_gpu_lyapunov.py), recorded on the GPU from the library as it is built:

    python tests/golden/make_tangent_norm_fixture.py

It was run once, at e2fbb09: the commit before the norm became the inner product of perturbation 0 with itself, while the norm had
a kernel of its own beside k_tangent_dot.  The grids and the sequence of calls are tests/tangent_norm_cases.py's; each grid is run on a fresh
Model and written to tests/golden/tangent_norm_bits.json as

  nx, ny, kind              the grid and the norm's kind
  set, stepped, rescaled    the uint64 bits of tangent_norm after set_tangent, after 2 steps and after rescale_tangent(-1.75)
  gram                      on the first three grids: the uint64 bits of tangent_gram of a set of three, row-major
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]


def make():
    import tangent_norm_cases as N
    out = []
    for nx, ny in N.GRIDS:
        m = N.model(nx, ny)
        got = N.bits(m, nx, ny)
        m.close()
        for kind, e in got.items():
            out.append(dict({"nx": nx, "ny": ny, "kind": kind}, **e))
            print(json.dumps(out[-1]))
    with open(os.path.join(HERE, "tangent_norm_bits.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e) for e in out) + "\n]\n")
    print("%d entries" % len(out))


if __name__ == "__main__":
    make()
