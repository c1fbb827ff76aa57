#!/usr/bin/env python3
"""The refusal table of the model/slab entry points (tests/test_gpu_entry.py), recorded on the GPU from the library as it is built:

    python tests/golden/make_entry_fixture.py

It was run twice: at 321421f, the commit before the entry points were given one body per pair and one guard layer, so the table holds
what the hand-written pairs returned; and at e2fbb09, the commit before the single tangent became the subspace of one, with the five
pairs of the tangent subspace added to tests/entry_cases.py.  An entry that the file already holds with the status that the call
returns now is kept as it was first recorded, so the second table differs from the first by the added entries alone (twelve of the
earlier messages, which the test does not compare, were reworded when every entry point came to name itself).  The calls and their argument recipes are tests/entry_cases.py's; each is made on Model(64) or on an
unconnected slab (rank 0 of world 2) and written to tests/golden/entry_refusals.json as

  fn, args      the function and its argument recipe
  rc            the status it returned
  phrase        the part of its message that tells this refusal from the others ("" for a set-up call, which returns FB_OK)
  message       the whole message, for the reader; the test does not compare it
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def make():
    import entry_cases as E
    path = os.path.join(HERE, "entry_refusals.json")
    earlier = {(e["fn"], json.dumps(e["args"]), e["rc"], e["phrase"]): e for e in json.load(open(path))}
    h = E.Handles()
    out = []
    try:
        for fn, args, phrase in E.ENTRIES:
            rc, msg = h.call(fn, args)
            assert (rc == 0) == (phrase == ""), (fn, args, rc, msg)
            assert phrase in msg, (fn, args, phrase, msg)
            e = {"fn": fn, "args": args, "rc": rc, "phrase": phrase, "message": msg if rc else ""}
            out.append(earlier.get((fn, json.dumps(args), rc, phrase), e))      # what an earlier run recorded stays, its message too
            print("%-40s %-50s -> %d %s" % (fn, json.dumps(args), rc, msg if rc else ""))
    finally:
        h.close()
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e) for e in out) + "\n]\n")
    print("%d entries" % len(out))


if __name__ == "__main__":
    make()
