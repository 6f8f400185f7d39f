"""A training iteration of the per-pair baselines CNN, PCNN and LSTM at the reference's widths, from device-resident data
(`recon_amd.run_epoch` over a `PairData`) and by the hand-written loop of train.py (host slices, `astype`, pageable uploads, the status
word read in every forward), in one process.

A synthetic dataset of N = 10 000 rows of T = 36 tokens in each of the three forms (tests/pair_data_checks.py), 2 000 words of 50, n_out =
353, the models with model_params.json's sizes (units1 256, position_emb 3, window_size 3, dropout1 0.5), in train mode,
`recon_amd.optim.Adam(max_grad_norm=0.25)`, batches of 50.  The legs, alternating round by round (round 0 warms up and is dropped; every
timing is an epoch's wall clock ending in a synchronize, over its 200 iterations, so that the shortest leg, `take` alone, still times
milliseconds of work):

    a  run_epoch: a training epoch
    b  the hand-written loop, the same
    c  `take` alone over the epoch's batches: the kernel, torch indexing of the device-resident arrays, host slices plus uploads
    d  (a) with the status word read in every forward (`ids_prechecked` left out): what the once-per-epoch id check is worth

    python tools/pair_epoch_bench.py [--rounds 7] [--out profiles/pair_epoch_bench.jsonl]
"""
import argparse
import contextlib
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

from op_bench import put_ms, write_lines  # noqa: E402
from pair_data_checks import dataset, hand_written  # noqa: E402
from stage_a_iter_bench import count_launches  # noqa: E402

# the reference's model_params.json (the keys the three models read)
PARAMS = {"dropout1": 0.5, "position_emb": 3, "units1": 256, "rnn1": "LSTM", "rnn1_layers": 1, "bidirectional": 1, "window_size": 3}
N_OUT, N_WORDS, WORD_DIM, T = 353, 2000, 50, 36
MODELS = {"CNN": "positions", "PCNN": "segments", "LSTM": "marks"}


def make_model(name, dev):
    import recon_amd
    torch.manual_seed(0)
    emb = np.random.RandomState(0).randn(N_WORDS, WORD_DIM).astype(np.float32)
    m = getattr(recon_amd, name)(dict(PARAMS), emb, T, N_OUT)
    m.packed_word_dropout = True
    return m.to(dev).train()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from recon_amd import PairData, RelationMetrics, pair_data, run_epoch, stage_b
    from recon_amd.optim import Adam
    dev = torch.device("cuda:0")
    N, bs = a.rows, a.batch
    iters = N // bs
    order = np.random.default_rng(1).permutation(N).astype(np.int64)
    order_d = torch.from_numpy(order).to(dev)
    metrics = RelationMetrics(dev)
    legs, launches, lines = {}, {}, []

    def add(name, form, seed):
        as_indices = dataset(N, T, form, seed, n_words=N_WORDS, n_out=N_OUT)
        data = PairData.from_indices(as_indices).to(dev)
        model = make_model(name, dev)
        opt = Adam(filter(lambda p: p.requires_grad, model.parameters()), lr=1e-4, weight_decay=0, max_grad_norm=0.25)

        def leg_a():
            run_epoch(model, data, bs, order=order_d, optimizer=opt, metrics=metrics)

        def leg_b():
            hand_written(model, as_indices, bs, order, opt, metrics, None, dev)

        def leg_d():
            prev, stage_b.ids_prechecked = stage_b.ids_prechecked, contextlib.nullcontext
            try:
                run_epoch(model, data, bs, order=order_d, optimizer=opt, metrics=metrics)
            finally:
                stage_b.ids_prechecked = prev

        def take_kernel():
            for i in range(iters):
                data.take(order_d, i * bs, bs)

        def take_torch():
            prev, pair_data._KERNELS = pair_data._KERNELS, False
            try:
                for i in range(iters):
                    data.take(order_d, i * bs, bs)
            finally:
                pair_data._KERNELS = prev

        def take_host():
            for i in range(iters):
                at = order[i * bs:(i + 1) * bs]
                torch.from_numpy(as_indices[0][at].astype(int)).to(dev)
                torch.from_numpy(as_indices[1][at].astype(int)).to(dev)
                torch.from_numpy(as_indices[2][at].astype(int)).view(-1).to(dev)
                if form == "segments":
                    torch.from_numpy(np.array(as_indices[3][at])).float().to(dev)
        legs.update({name + "_a_run_epoch": leg_a, name + "_b_hand_written": leg_b, name + "_d_read_per_forward": leg_d,
                     name + "_c_take_kernel": take_kernel, name + "_c_take_torch": take_torch, name + "_c_take_host": take_host})
        launches.update({name + "_a": leg_a, name + "_b": leg_b})
        return data

    datas = {name: add(name, form, 2024 + i) for i, (name, form) in enumerate(MODELS.items())}
    times = {k: [] for k in legs}
    for rnd in range(a.rounds + 1):
        for k, fn in legs.items():
            ms = wall(fn) / iters
            if rnd:
                times[k].append(ms)
        metrics.reset()
    for name, form in MODELS.items():
        line = {"tool": "pair_epoch_bench", "device": torch.cuda.get_device_name(0), "model": name, "form": form, "N": N, "B": bs, "T": T, "n_out": N_OUT,
                "units1": PARAMS["units1"], "iterations_per_epoch": iters, "rounds": a.rounds,
                "unit": "ms per iteration (an epoch's wall clock, ending in a synchronize, over its iterations)",
                "dataset_device_bytes": sum(t.numel() * t.element_size() for t in datas[name].arrays.values())}
        for k, v in times.items():
            if k.startswith(name + "_"):
                put_ms(line, k[len(name) + 1:] + "_ms", v)
                if k.endswith(("_a_run_epoch", "_b_hand_written", "_d_read_per_forward")):
                    line[k[len(name) + 1:] + "_ms_rounds"] = [round(x, 4) for x in v]          # these legs are host-paced: their spread is part of the result
        for leg in ("a", "b"):
            n = count_launches(launches[name + "_" + leg], iters=1)
            line[leg + "_launches_per_iteration"] = None if n is None else round(n / iters, 1)
        line["b_over_a_median"] = round(line["b_hand_written_ms_median"] / line["a_run_epoch_ms_median"], 4)
        line["d_over_a_median"] = round(line["d_read_per_forward_ms_median"] / line["a_run_epoch_ms_median"], 4)
        line["a_median_below_b_min"] = line["a_run_epoch_ms_median"] < line["b_hand_written_ms_min"]
        line["a_median_below_d_min"] = line["a_run_epoch_ms_median"] < line["d_read_per_forward_ms_min"]
        # the wiring rule: the kernel is the default where its median lies below the torch-primitive form's minimum in the same process
        line["take_kernel_median_below_torch_min"] = line["c_take_kernel_ms_median"] < line["c_take_torch_ms_min"]
        line["take_kernel_median_below_host_min"] = line["c_take_kernel_ms_median"] < line["c_take_host_ms_min"]
        lines.append(json.dumps(line))
        print(lines[-1])
    write_lines(a.out, lines)


if __name__ == "__main__":
    main()
