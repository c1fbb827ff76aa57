#!/usr/bin/env python3
"""The bits of everything stepped beside the vorticity (tests/test_gpu_beside_bits.py), recorded on the GPU from the library as it is built:

    python tests/golden/make_beside_bits_fixture.py

It was run once, at b678974: the commit before csrc/fb_beside.h was split by model and its transform passes, its variable sets and its
allocations went through shared helpers.  The grids and the sequence of calls are tests/beside_bits_cases.py's; each grid is run twice,
each time on a fresh Model, and an output whose two digests differ is left out (and named on stderr).  Written to
tests/golden/beside_bits.json as one entry per grid:

  nx, ny      the grid
  sha256      by the output's name, the SHA-256 of its bytes

beside_bits_cases.CHUNK = 8 restates ADJOINT_CHUNK (csrc/fb_adjoint.h) and REPLAY_CHUNK (csrc/fb_replay.h), which Python cannot read:
the sets of CHUNK + 1 on 256^2 are there so that the second chunk is a chunk of one.  If either constant changes, change CHUNK with it
and record the fixture again, or that case is no longer run and nothing says so.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]


def make():
    import beside_bits_cases as B
    out = []
    for nx, ny in B.GRIDS:
        runs = []
        for _ in range(2):
            m = B.model(nx, ny)
            runs.append(B.digests(m, nx, ny))
            m.close()
        keep = {k: v for k, v in runs[0].items() if runs[1][k] == v}
        for k in runs[0]:
            if k not in keep:
                print("%dx%d: %s differs between two runs: left out" % (nx, ny, k), file=sys.stderr)
        out.append({"nx": nx, "ny": ny, "sha256": keep})
        print(json.dumps(out[-1]))
    with open(os.path.join(HERE, "beside_bits.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e) for e in out) + "\n]\n")
    print("%d grids, %d digests" % (len(out), sum(len(e["sha256"]) for e in out)))


if __name__ == "__main__":
    make()
