#!/usr/bin/env python3
"""Writes the shipped maps as the map.bin files tools/field_probe.cpp reads, builds the probe and runs it on each: lookups per
beam, trips per wave and the trip histogram of the quadrant and the octant free-rectangle fields (host only, no GPU).

    python tools/field_probe.py [robots] > profiles/octant_field/field_probe.txt
"""
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-collision-avoidance_amd"))
from mrca import scenario as S  # noqa: E402

BUILD = os.path.join(ROOT, "tools", "_build")
# map, half side of the square the poses are drawn from (Stage-1: the 9 m disc's square; the others: most of the map)
MAPS = (("stage1", lambda: S.stage1(1, 2).grid, 9.0), ("stage2", lambda: S.stage2(1).grid, 19.0), ("circle", lambda: S.circle(1).grid, 28.0))


def main():
    robots = sys.argv[1] if len(sys.argv) > 1 else "3000"
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "field_probe")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-pthread",
                    os.path.join(ROOT, "tools", "field_probe.cpp"), "-o", exe], check=True)
    for name, make, half in MAPS:
        g = make()
        path = os.path.join(BUILD, f"field_probe_{name}.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<iiifff", g.width, g.height, g.words_per_row, g.cell, g.x0, g.y0))
            f.write(np.ascontiguousarray(g.bits, np.uint32).tobytes())
        print(f"## {name}", flush=True)
        subprocess.run([exe, path, robots, str(half)], check=True)
        print(flush=True)


if __name__ == "__main__":
    main()
