#!/usr/bin/env python3
"""Record what mrca_arena_bytes answers to every config of tests/arena_layout_cases.py: tests/golden/arena_layout.json, {case:
[return code, bytes]} or, for a config it refuses, {case: [return code, mrca_last_error()]}, from the library as it is built now
(no GPU needed: mrca_arena_bytes touches no device).  tests/test_arena_layout_host.py replays the cases against the file.  Run it
on the commit whose layout is to be kept, BEFORE a change to the arena's description -- not after, to make a failing test pass."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rl-collision-avoidance_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "golden", "arena_layout.json")


def main():
    import __graft_entry__ as g
    g.build()
    from mrca import _lib
    import arena_layout_cases
    got = arena_layout_cases.record(_lib.load())
    with open(OUT, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    with open(OUT, "rb") as f:
        print(f"{len(got)} cases -> {OUT}  sha256 {hashlib.sha256(f.read()).hexdigest()}")


if __name__ == "__main__":
    main()
