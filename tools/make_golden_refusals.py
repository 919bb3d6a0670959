#!/usr/bin/env python3
"""Record what the controllers' entry points answer to bad arguments: tests/golden/abi_refusals.json, {case: [return code,
mrca_last_error()]} for every case of tests/abi_refusal_cases.py, from the library as it is built now (no GPU needed: every
call is refused before a launch).  tests/test_abi_refusals_host.py replays the cases against the file.  Run it on the commit
whose behaviour is to be kept, BEFORE a change to the host layer -- not after, to make a failing test pass."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rl-collision-avoidance_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "golden", "abi_refusals.json")


def main():
    import __graft_entry__ as g
    g.build()
    from mrca import _lib
    import abi_refusal_cases
    got = abi_refusal_cases.record(_lib.load())
    with open(OUT, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} cases -> {OUT}")


if __name__ == "__main__":
    main()
