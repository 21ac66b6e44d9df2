"""Recorder of tests/golden/nn_parent.json, the fixture of tests/test_nn_parent_bits.py (needs a GPU).

Run it on builds of the PARENT commit's three NN libraries (libvboc_fit.so, libvboc_cls.so, libvboc_pool.so in one
directory inside the repository, e.g. vboc_amd/variants/nn_parent/): the fixture pins every output of the commit before
the libraries' forward passes were shared, and the test compares the tree's libraries with it bit for bit.  The cases,
their inputs and their weights are the test module's own (seeded NumPy generators); this tool only points the ctypes
modules at the given directory, runs every case twice and writes, per output array, its sha1, dtype, shape and first 8
values (the sha1 alone for the cases in HASH_ONLY).  A case whose two runs differ is reported and left out.

usage: python tools/record_nn_parent.py --libdir vboc_amd/variants/nn_parent [--out file.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libdir", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "nn_parent.json"))
    a = ap.parse_args()
    import torch   # before the libraries are loaded: torch brings its own HIP runtime
    assert torch.cuda.is_available(), "the recorder needs a GPU"
    from vboc_amd import clslib, fitlib, poollib
    for mod, name in ((fitlib, "libvboc_fit.so"), (clslib, "libvboc_cls.so"), (poollib, "libvboc_pool.so")):
        mod.LIB_PATH = os.path.join(os.path.abspath(a.libdir), name)
        assert os.path.exists(mod.LIB_PATH), mod.LIB_PATH
        mod.load()
    import test_nn_parent_bits as T
    cases, dropped = {}, []
    for name in T.CASES:
        first, second = T.digest(T.run_case(name)), T.digest(T.run_case(name))
        if first != second:
            dropped.append(name)
            print(f"NOT REPRODUCIBLE on the parent itself, left out: {name}")
            continue
        if name in T.HASH_ONLY:
            for v in first.values():
                del v["head"]
        cases[name] = first
    with open(a.out, "w") as f:        # one line per case
        f.write('{"device": %s,\n "cases": {\n' % json.dumps(torch.cuda.get_device_name(0)))
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in sorted(cases.items())))
        f.write("\n }}\n")
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, {len(cases)} cases, dropped {dropped}")


if __name__ == "__main__":
    main()
