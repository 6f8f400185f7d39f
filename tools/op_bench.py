"""What the fused encoder ops' bench tools (char_features_bench, ctx_lstm_bench, sent_lstm_bench, transitions_bench, translation_bench)
share: the timing of one forward + backward, the rounds, the summary fields, the wiring rule's field and the JSONL append.  A path is a
function without arguments that returns the output tensor, or a list of them; `g_out` is the matching gradient or list of gradients."""
import statistics

import torch


def _backward(out, g_out):
    if torch.is_tensor(out):
        out.backward(g_out)
    else:
        torch.autograd.backward(list(out), g_out)


def timed(fn, g_out):
    """(forward ms, forward + backward ms, peak bytes above what was allocated before) of fn() and its backward."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    out = fn()
    e[1].record()
    _backward(out, g_out)
    e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[0].elapsed_time(e[2]), torch.cuda.max_memory_allocated() - base


def timed_forward(fn):
    """Milliseconds of fn() under no_grad."""
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    with torch.no_grad():
        fn()
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1])


def launches(fn, g_out):
    """Device-side events (kernels, memsets, copies) of one forward + backward, or None where the profiler is not available."""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            _backward(fn(), g_out)
            torch.cuda.synchronize()
        return sum(1 for ev in prof.events() if ev.device_type == DeviceType.CUDA)
    except Exception:                                                      # the count is a by-product: the timings do not depend on it
        return None


def run_rounds(paths, g_out, clear_grads, rounds, nograd=None):
    """{path: [timed(...) per round]} and the no_grad forward times of `nograd` (one per round, after the paths).  Round 0 warms up and is
    dropped; the paths alternate within a round; `clear_grads()` runs before each timing."""
    res, plain = {k: [] for k in paths}, []
    for rnd in range(rounds + 1):
        for k, fn in paths.items():
            clear_grads()
            r = timed(fn, g_out)
            if rnd:
                res[k].append(r)
        if nograd is not None:
            t = timed_forward(nograd)
            if rnd:
                plain.append(t)
    return res, plain


def put_ms(line, key, values):
    values = list(values)
    line[key + "_median"] = round(statistics.median(values), 4)
    line[key + "_min"] = round(min(values), 4)


def summarise(line, res, paths, g_out, clear_grads):
    """Per path the *_fwd_ms_*, *_fwd_bwd_ms_*, *_peak_bytes and *_launches_fwd_bwd fields, then speedup_fwd_bwd_median."""
    for k, rs in res.items():
        put_ms(line, k + "_fwd_ms", (r[0] for r in rs))
        put_ms(line, k + "_fwd_bwd_ms", (r[1] for r in rs))
        line["%s_peak_bytes" % k] = max(r[2] for r in rs)
        clear_grads()
        line["%s_launches_fwd_bwd" % k] = launches(paths[k], g_out)
    line["speedup_fwd_bwd_median"] = round(line["chain_fwd_bwd_ms_median"] / line["op_fwd_bwd_ms_median"], 3)


def wiring_rule(line):
    """The rule under which a model may call the op by default: its median forward + backward lies below the chain's minimum."""
    line["op_median_below_chain_min"] = line["op_fwd_bwd_ms_median"] < line["chain_fwd_bwd_ms_min"]


def write_lines(path, lines, mode="a"):
    if path:
        with open(path, mode) as f:
            f.write("\n".join(lines) + "\n")
