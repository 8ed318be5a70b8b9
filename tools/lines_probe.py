"""The random-line ceiling under the pipelined calls' conditions: probe.hip's kernel (two
random 128-byte lines and 8 bytes of request per check, nothing else) launched round-robin on
1 and on 2 streams (ketogpu_probe_random_lines_streams), time per launch.

    python tools/lines_probe.py [--requests 1000000] [--table-gib 2] [--reps 40]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from keto_amd import _lib as L  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--requests", type=int, default=1_000_000)
p.add_argument("--table-gib", type=float, default=2.0)
p.add_argument("--reps", type=int, default=40)
a = p.parse_args()
out = {"requests": a.requests, "table_bytes": int(a.table_gib * (1 << 30)), "reps": a.reps}
for streams in (1, 2):
    ms = C.c_double(0)
    L.check(L.lib().ketogpu_probe_random_lines_streams(0, out["table_bytes"], a.requests, a.reps, streams, C.byref(ms)))
    out[f"us_per_launch_{streams}_streams"] = round(ms.value * 1e3, 2)
print(json.dumps(out))
