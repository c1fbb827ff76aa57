#!/usr/bin/env python3
"""Generates tests/golden/ref_io.npz.  Run where oracle/_ref is built (the build container), after __graft_entry__.build().

What the REFERENCE's own host programs, compiled unmodified into oracle/_ref, write for the inputs of the tests that compare
the product and the oracle against them, so that those tests need no oracle/_ref.  Data only; byte strings are stored as uint8.
  fieldio_rng1_1000          : writeField (fieldio.cpp:7-19) of tests/test_oracle.py::test_fieldio_bytes_match_reference_library's array
  fieldio_rng7_12345[_stderr]: file and stderr of tests/test_host_cpp.py's _FIELDIO_CHILD on the reference's libfieldio.so
  fifo_stream                : vort_src_input.out at its compiled-in configuration (vort_src_input.cpp:35-61)
  find_min_std{out,err}      : find_min.out (find_min.cpp:67-101) on tests/test_host_cpp.py's _find_min_input
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import test_host_cpp as H  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")


def u8(b):
    return np.frombuffer(b, dtype=np.uint8).copy()


def main():
    out = {}
    with tempfile.TemporaryDirectory() as d:
        lib = ctypes.CDLL(os.path.join(REF, "libfieldio.so"))
        wr = getattr(lib, "_Z10writeFieldPKcPfm")
        wr.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_float), ctypes.c_size_t]
        wr.restype = None
        a = np.random.default_rng(1).standard_normal(1000).astype(np.float32)
        p = os.path.join(d, "ref.bin")
        wr(p.encode(), a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), a.size)
        out["fieldio_rng1_1000"] = u8(open(p, "rb").read())

        import pathlib
        data, err = H._run_fieldio_child(os.path.join(REF, "libfieldio.so"), pathlib.Path(d) / "child")
        out["fieldio_rng7_12345"], out["fieldio_rng7_12345_stderr"] = u8(data), u8(err)

        out["fifo_stream"] = u8(subprocess.run([os.path.join(REF, "vort_src_input.out")], cwd=d, stdout=subprocess.PIPE,
                                               stderr=subprocess.DEVNULL, check=True).stdout)

        _, inp = H._find_min_input(d)
        res = subprocess.run([os.path.join(REF, "find_min.out")], cwd=d, input=inp.encode(), stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, check=True)
        out["find_min_stdout"], out["find_min_stderr"] = u8(res.stdout), u8(res.stderr)
    np.savez_compressed(os.path.join(HERE, "ref_io.npz"), **out)
    print("wrote", os.path.join(HERE, "ref_io.npz"), {k: v.size for k, v in out.items()})


if __name__ == "__main__":
    main()
