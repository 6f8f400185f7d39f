"""Wall clock of one stage-B entity-context batch, from the [B, C, 2] ids to device-resident model inputs, by three paths in one process:
the kernels (csrc/ctx_batch.hip), the same results from torch primitives, and the plain-loop host restatement of
tests/context_batch_checks.py plus the uploads of its arrays — the stand-in for the reference's train.py:250-273 — once tokenising
every line in every batch, as the reference does, and once with each entity's token lists kept between batches.

A synthetic dataset at the reference's scale: a 50 x 72 batch, Zipf ids with about 450 unique entities, contexts of 1-32 lines, G = 100.
Per path: median and minimum over the rounds (round 0 warms up and is dropped; the device paths alternate inside a round; every timing
ends with a synchronize), device launches and copies of one call (torch.profiler), host reads, and the peak bytes above the outputs.

    python tools/context_batch_bench.py [--rounds 20] [--host-rounds 3] [--out profiles/context_batch_bench.jsonl]
    rocprofv3 --kernel-trace --stats -- python tools/context_batch_bench.py --loop 50       # kernel times, a run of its own
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from context_batch_checks import build, random_batch, random_dataset, restate  # noqa: E402
from op_bench import put_ms, write_lines  # noqa: E402


def make_case(B, Cn, G, want_unique, seed):
    rng = np.random.default_rng(seed)
    ds = random_dataset(rng, 1500, G)
    best = None
    for zipf in (1.05, 1.1, 1.15, 1.2, 1.3, 1.4, 1.6):
        ids, sf = random_batch(np.random.default_rng(seed + 1), ds, B, Cn, zipf=zipf)
        u = len(np.unique(ids))
        if best is None or abs(u - want_unique) < abs(best[0] - want_unique):
            best = (u, zipf, ids, sf)
    return ds, best


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def device_events(fn):
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for ev in prof.events() if ev.device_type == DeviceType.CUDA)
    except Exception:
        return None


def output_bytes(batch):
    ts = (batch.unique_entities, batch.entities_position, batch.context_words, batch.context_chars, batch.context_mask, batch.gat_entity_embeddings,
          batch.nonzero_gat_entity_embeddings, batch.nonzero_entity_pos)
    return sum(t.numel() * t.element_size() for t in ts if t is not None)


def peak_above_outputs(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base - output_bytes(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--pairs", type=int, default=72)
    ap.add_argument("--gat-dim", type=int, default=100)
    ap.add_argument("--unique", type=int, default=450)
    ap.add_argument("--int32", action="store_true", help="context_words / context_chars as int32")
    ap.add_argument("--loop", type=int, default=0, help="only run the kernel path this many times (for a profiler)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from recon_amd import ContextBatcher, context_batch
    dev = torch.device("cuda:0")
    ds, (n_unique, zipf, ids, sf) = make_case(a.batch, a.pairs, a.gat_dim, a.unique, 2024)
    t0 = time.perf_counter()
    tables, surface_ids = build(ds, "wikidata", sf, "selected")
    build_ms = (time.perf_counter() - t0) * 1e3
    batcher = ContextBatcher(tables.to(dev))
    ids_d, sid_d = torch.from_numpy(ids).to(dev), torch.from_numpy(surface_ids).to(dev)
    dtype = torch.int32 if a.int32 else torch.int64

    def kernels():
        return batcher.batch(ids_d, sid_d, index_dtype=dtype)

    def stock():
        prev, context_batch._KERNELS = context_batch._KERNELS, False
        try:
            return batcher.batch(ids_d, sid_d, index_dtype=dtype)
        finally:
            context_batch._KERNELS = prev

    if a.loop:
        for _ in range(a.loop):
            kernels()
        torch.cuda.synchronize()
        return

    def host(cache):
        r = restate(ds, "wikidata", ids, sf, "selected", cached_lines=cache)
        up = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in r.items() if isinstance(v, np.ndarray)}
        if a.int32:
            up["words"], up["chars"] = up["words"].to(torch.int32), up["chars"].to(torch.int32)
        return up

    times = {"kernels": [], "torch": []}
    for rnd in range(a.rounds + 1):
        for name, fn in (("kernels", kernels), ("torch", stock)):
            ms, _ = wall(fn)
            if rnd:
                times[name].append(ms)
    cache = {}
    host(cache)                                                         # fills the cache; also the host paths' warm-up
    host_t = {"host_tokenising": [], "host_cached_tokens": []}
    for _ in range(a.host_rounds):
        host_t["host_tokenising"].append(wall(lambda: host(None))[0])
        host_t["host_cached_tokens"].append(wall(lambda: host(cache))[0])
    b = kernels()
    line = {"tool": "context_batch_bench", "device": torch.cuda.get_device_name(0), "B": a.batch, "C": a.pairs, "ids": int(ids.size), "G": a.gat_dim,
            "unique": int(b.unique_entities.numel()), "zipf": zipf, "P_b": b.context_words.shape[1], "T_b": b.context_words.shape[2],
            "index_dtype": "int32" if a.int32 else "int64", "output_bytes": output_bytes(b), "char_block_bytes": b.context_chars.numel() * b.context_chars.element_size(),
            "tables_bytes": sum(t.numel() * t.element_size() for t in tables.arrays.values()), "tables_build_ms": round(build_ms, 1),
            "rounds": a.rounds, "host_rounds": a.host_rounds}
    for k, v in list(times.items()) + list(host_t.items()):
        put_ms(line, k + "_ms", v)
    line["kernels_device_events"], line["torch_device_events"] = device_events(kernels), device_events(stock)
    line["kernels_host_reads"] = 1
    line["kernels_peak_bytes_above_outputs"], line["torch_peak_bytes_above_outputs"] = peak_above_outputs(kernels), peak_above_outputs(stock)
    line["speedup_vs_host_tokenising_median"] = round(line["host_tokenising_ms_median"] / line["kernels_ms_median"], 1)
    line["speedup_vs_host_cached_tokens_median"] = round(line["host_cached_tokens_ms_median"] / line["kernels_ms_median"], 1)
    line["torch_over_kernels_median"] = round(line["torch_ms_median"] / line["kernels_ms_median"], 2)
    line["kernels_median_below_torch_min"] = line["kernels_ms_median"] < line["torch_ms_min"]
    text = json.dumps(line)
    print(text)
    write_lines(a.out, [text])


if __name__ == "__main__":
    main()
