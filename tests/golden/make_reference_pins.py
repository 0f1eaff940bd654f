#!/usr/bin/env python3
"""Records what the reference's own host code answers — oracle/_ref/libtc_ref.so (Surface geometry, converter dispatch) and
oracle/_ref/libtc_core_ref.so (Token / Task state machine), both compiled by oracle/Makefile from the reference tree — into

  tests/golden/reference_tc_pins.json          every probe / geometry query tests/test_reference_tc_pin.py makes
  tests/golden/reference_tc_core_traces.json   every call sequence of tests/test_tc_core_vs_reference.py

so that those tests compare this repo with the reference where oracle/_ref cannot be built.  Needs oracle/_ref (`python -c "import oracle;
oracle.build()"` where the reference tree is) and the built PyNvCodec.

  python tests/golden/make_reference_pins.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_reference_tc_pin as pin  # noqa: E402
import test_tc_core_vs_reference as core  # noqa: E402

SIZES = [(1920, 1080), (848, 464), (64, 32), (3840, 2160), (7, 5)]


def main():
    ref = core.load_ref()
    if pin.REF is None or ref is None:
        raise SystemExit("oracle/_ref is not built: build it where the reference tree is (oracle/Makefile)")
    ctxs = [(-1, -1)] + [(cs, cr) for cs in range(3) for cr in range(3)]
    pins = {"probe": {f"{i},{o},{cs},{cr}": pin.live_probe(i, o, cs, cr) for i in range(1, 14) for o in range(1, 14) for cs, cr in ctxs},
            "geometry": {f"{f},{w},{h}": pin.live_geometry(f, w, h) for w, h in SIZES for f in range(1, 18)}}
    traces = {str(seed): core.trace(ref, seed) for seed in core.SEEDS}
    for path, obj in ((pin.GOLDEN, pins), (core.GOLDEN, traces)):
        with open(path, "w") as f:
            json.dump(obj, f, separators=(",", ":"), sort_keys=True)
            f.write("\n")
        print(f"wrote {os.path.relpath(path, ROOT)}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
