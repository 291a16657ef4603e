#!/usr/bin/env python3
"""bench.py's config-3 MLP SGHMC leg alone (bench.mlp_measure: 784-256-256-10, B = 500, float32, 40 steps, three
timed calls): one line with the median call's rate in leapfrogs per device millisecond and every call's beside it.
For an A/B of two builds run it once per process with HMCX_LIB naming the library file under lib/, in alternating
pairs (the order within a pair alternating too):
    HMCX_LIB=libhmcx_parent.so python tools/mlp_sghmc_leg.py; HMCX_LIB=libhmcx.so python tools/mlp_sghmc_leg.py; ..."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import bench  # noqa: E402


def main():
    X, Y = bench.synthetic_data(0)
    out = bench.mlp_measure(X, np.argmax(Y, axis=1), 40, 0)
    rates = sorted(r["leapfrogs"] / r["device_ms"] for r in out["runs"])
    print("[%s] median %.2f leapfrog/device-ms (calls %s)" % (os.environ.get("HMCX_LIB", "libhmcx.so"), rates[1],
                                                                ", ".join("%.2f" % r for r in rates)), flush=True)


if __name__ == "__main__":
    main()
