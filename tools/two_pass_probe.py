#!/usr/bin/env python3
"""Does a 34 MB / 1 GiB write-through stream cost more when it leaves in TWO passes of aligned blocks?

mrl_probe_stream mode 2 (one pass of 16-byte sc1 stores) against modes 3 / 4 (the same bytes and stores in two passes inside
one launch: first a fixed pseudo-random quarter of the aligned 64- / 128-byte blocks, then the rest), alternating on the same
buffer in one process.  A block size is "free" if its median is within the spread (max - min) of mode 2's own repetitions.
`python tools/two_pass_probe.py [out.json]` (profiles/r05_a_two_pass_store_probe.txt)."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madrona_rl_envs_playground_amd import _lib  # noqa: E402

REPS = 7
L = _lib.lib()
stream = torch.cuda.current_stream().cuda_stream
buf = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def us_per_launch(mode, nbytes, launches):
    def launch():
        _lib.check(L.mrl_probe_stream(buf.data_ptr(), buf.data_ptr(), nbytes, mode, 0, stream))
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(launches):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


out = {"build": _lib.build_hash(), "sizes": {}}
MODES = ((2, "one_pass"), (3, "two_pass_64B"), (4, "two_pass_128B"))
# 32768 worlds of cramped_room (inside the 256 MiB Infinity Cache) and 1 GiB (beyond it)
for name, nbytes, launches in (("34MB", 32768 * 1040, 400), ("1GiB", 1 << 30, 12)):
    runs = {m: [] for m, _ in MODES}
    for _ in range(REPS):
        for m, _ in MODES:
            runs[m].append(us_per_launch(m, nbytes, launches))
    base = runs[2]
    spread = max(base) - min(base)
    d = {"one_pass_spread_us": round(spread, 3)}
    for m, label in MODES:
        v = runs[m]
        d[label] = {"us": [round(x, 3) for x in v], "median_us": round(statistics.median(v), 3),
                    "TBps": round(nbytes / statistics.median(v) / 1e6, 3)}
        if m != 2:
            excess = statistics.median(v) - statistics.median(base)
            d[label].update(excess_us=round(excess, 3), free=bool(excess <= spread))
    out["sizes"][name] = d
    print(name, json.dumps(d), flush=True)
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
