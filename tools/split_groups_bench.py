"""Kernel times of outputs per read group (README "Outputs per read group"): rd_gz_compress_grouped and rd_group_pack at K = 2 x 25 and
2 x 385 keys, uniform over the groups, against TWO rd_gz_compress_selected / rd_select_pack calls - what the unsplit run does - over
the same resident chunk of 2^20 records of 100 bp. One process, the legs alternating, device events around 20 calls a leg, one
warm-up round and three timed ones: median, lowest and highest. Prints one JSON line per K (profiles/split_groups_bench.jsonl).
  python tools/split_groups_bench.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ribodetector_amd import _native as N  # noqa: E402
from ribodetector_amd.gz import DeviceGroupSelect, DeviceGzip, DeviceSelect  # noqa: E402

DEV = "cuda:0"
n, L = 1 << 20, 100
rng = np.random.default_rng(1)
rec = np.empty((n, 9 + L + 3 + L + 1), dtype=np.uint8)
ids = np.char.zfill(np.arange(n).astype("U7"), 7)
rec[:, 0] = ord("@")
rec[:, 1:8] = np.frombuffer("".join(ids).encode(), dtype=np.uint8).reshape(n, 7)
rec[:, 8] = 10
rec[:, 9:9 + L] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, L))]
rec[:, 9 + L:12 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
rec[:, 12 + L:12 + 2 * L] = np.frombuffer(b"F:,#", dtype=np.uint8)[rng.choice(4, (n, L), p=[0.9, 0.06, 0.03, 0.01])]
rec[:, -1] = 10
text = torch.from_numpy(rec.reshape(-1)).to(DEV)
rs = torch.arange(n + 1, dtype=torch.int64, device=DEV) * rec.shape[1]
labels = torch.from_numpy(rng.integers(0, 2, n).astype(np.int8)).to(DEV)
tb = int(text.numel())
gs, dg, ds = DeviceGroupSelect(DEV), DeviceGzip(DEV), DeviceSelect(DEV)


def timed(fn, calls=20):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


out = []
for G1 in (25, 385):
    K = 2 * G1
    keys = (labels.to(torch.int32) * G1 + torch.from_numpy(rng.integers(0, G1, n).astype(np.int32)).to(DEV)).contiguous()
    legs = {
        "gz_grouped": lambda: gs.compress_grouped(text, rs, keys, K, slot="g"),
        "gz_two_selected": lambda: (dg.compress_selected(text, rs, labels, 0, slot=0), dg.compress_selected(text, rs, labels, 1, slot=1)),
        "pack_grouped": lambda: gs.pack_grouped(text, rs, keys, K, slot="p"),
        "pack_two_selected": lambda: (ds.pack_selected(text, rs, labels, 0, slot=0), ds.pack_selected(text, rs, labels, 1, slot=1)),
    }
    ms = {k: [] for k in legs}
    for rnd in range(4):
        for k, fn in legs.items():
            t = timed(fn)
            if rnd:
                ms[k].append(round(t, 4))
    _, _, ginfo = gs.compress_grouped(text, rs, keys, K, slot="g")
    i0 = dg.compress_selected(text, rs, labels, 0, slot=0)[1]
    i1 = dg.compress_selected(text, rs, labels, 1, slot=1)[1]
    torch.cuda.synchronize()
    row = {"bench": "split_groups_kernels", "records": n, "text_bytes": tb, "K": K,
           "ms": {k: {"median": sorted(v)[1], "min": min(v), "max": max(v)} for k, v in ms.items()},
           "grouped_compressed_bytes": int(ginfo[0]), "grouped_members": int(ginfo[2]),
           "unsplit_compressed_bytes": int(i0[0]) + int(i1[0]), "unsplit_members": int(i0[2]) + int(i1[2]),
           "workspace_bytes_grouped_gz": int(N.lib().rd_group_workspace_bytes(n, tb, K, 1)), "workspace_bytes_gz": int(N.lib().rd_gz_workspace_bytes(n, tb))}
    out.append(row)
    print(json.dumps(row), flush=True)
