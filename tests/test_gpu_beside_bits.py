"""Everything stepped beside the vorticity gives the bits it gave before its host paths were rephrased through shared helpers (the
transform passes of csrc/fftbaro.hip, BesideSet, dev_alloc) and csrc/fb_beside.h was split by model: the tracer, the tangent set, the
particles with their deformation gradient, the adjoint and its set, the checkpointed window, the tangent replay, the observations and
the drifters' sweep, on the six grids of adjoint_numpy.PATH_CASES.  tests/beside_bits_cases.py makes the one sequence of calls;
tests/golden/beside_bits.json holds the SHA-256 of every output as tests/golden/make_beside_bits_fixture.py recorded them on the GPU
before the change.  An EngineSlab of one rank must give the Model's digests."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import beside_bits_cases as B                                   # noqa: E402

with open(os.path.join(HERE, "golden", "beside_bits.json")) as _f:
    FIXTURE = {(e["nx"], e["ny"]): e["sha256"] for e in json.load(_f)}
CASES = [(nx, ny, False) for nx, ny in B.GRIDS] + [(nx, ny, True) for nx, ny in B.SLAB_GRIDS]


def test_the_fixture_holds_every_grid():
    assert set(FIXTURE) == set(B.GRIDS)
    assert all(len(v) >= 20 for v in FIXTURE.values())
    assert {"adjoints.%d" % (B.CHUNK + 1), "replay.%d" % (B.CHUNK + 1)} <= set(FIXTURE[B.CHUNK_GRID])


@pytest.mark.parametrize("nx,ny,slab", CASES, ids=["%dx%d%s" % (nx, ny, "-slab" if slab else "") for nx, ny, slab in CASES])
def test_bits_are_the_recorded_ones(nx, ny, slab):
    m = B.model(nx, ny, slab)
    got = B.digests(m, nx, ny)
    m.close()
    want = FIXTURE[(nx, ny)]
    assert set(want) <= set(got)
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, "%dx%d: other bits than recorded: %s" % (nx, ny, differ)
