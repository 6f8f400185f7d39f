"""What recon_amd/gcn_layers.py asks of the library, call by call: a recorder around the handle `_lib.lib()` returns, and a grid of rows that
takes every branch of the file at the smallest shapes that reach it.

    python tools/probe/gcn_call_record.py --out DIR [--impl FILE]        # FILE: another gcn_layers.py, loaded under the package's name
    python tools/probe/gcn_call_record.py --compare DIR_A DIR_B           # records line for line, tensors bit for bit; exit status 1 on a difference

Every recon_gcn_* entry records its call, then calls through.  Of a struct passed by reference: every non-pointer field, for every pointer
field whether it is null (pointer arrays: entry by entry), and which pointer fields are equal to one another.  Of a size query: arguments and
answer.  Of the Python call: the exception's type and text, or shape, strides, storage offset and `_recon_padded` tag of every result and
gradient.  Results and gradients are saved to DIR/tensors.pt, the record to DIR/record.jsonl."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _struct(s, n_arrays):
    """Fields of a ctypes struct: values, null / set for pointers, entry-wise for pointer arrays (n_arrays entries), nested structs alike."""
    rec, ptrs = {}, {}
    for name, typ in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Structure):
            rec[name] = _struct(v, n_arrays)
        elif typ is C.c_void_p:
            rec[name] = "null" if not v else "set"
            if v:
                ptrs.setdefault(v, []).append(name)
        elif isinstance(v, C._Pointer):
            rec[name] = "null" if not v else ["null" if not v[i] else "set" for i in range(n_arrays)]
        else:
            rec[name] = v
    rec["equal_pointers"] = sorted(names for names in ptrs.values() if len(names) > 1)
    return rec


class Recorder:
    def __init__(self, real, symbols):
        self._real, self.calls = real, []
        self._argtypes = {name: args for name, _, args in symbols}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("recon_gcn_"):
            return fn

        def call(*args):
            rec = {"entry": name, "args": []}
            for a, typ in zip(args, self._argtypes[name]):
                if hasattr(a, "_obj"):                                   # byref(struct)
                    s = a._obj
                    rec["args"].append(_struct(s, getattr(s, "L", 0) or getattr(getattr(s, "fwd", None), "L", 0)))
                elif typ is C.c_void_p:
                    rec["args"].append("null" if not a else "set")
                else:
                    rec["args"].append(a)
            rec["returned"] = fn(*args)
            self.calls.append(rec)
            return rec["returned"]
        return call


def _meta(t):
    if t is None:
        return None
    return {"shape": list(t.shape), "strides": list(t.stride()), "offset": t.storage_offset(), "dtype": str(t.dtype),
            "padded": bool(getattr(t, "_recon_padded", False))}


class Session:
    def __init__(self, out_dir, impl):
        from recon_amd import _lib
        if impl:
            spec = importlib.util.spec_from_file_location("recon_amd.gcn_layers", impl)
            mod = importlib.util.module_from_spec(spec)
            sys.modules["recon_amd.gcn_layers"] = mod
            spec.loader.exec_module(mod)
        from recon_amd import gcn_layers, gat_layers
        self.lib, self.G, self.gat = _lib, gcn_layers, gat_layers
        self.rec = Recorder(_lib.lib(), _lib.SYMBOLS)
        _lib._lib = self.rec
        self.out_dir, self.lines, self.tensors = out_dir, [], {}
        self.dev = torch.device("cuda:0")

    def row(self, name, fn):
        """fn() -> result tensor(s), gradients included: recorded with the library calls it made, or the exception it raised."""
        self.rec.calls.clear()
        line = {"row": name}
        try:
            out = fn()
            outs = out if isinstance(out, (tuple, list)) else (out,)
            line["results"] = [_meta(t) for t in outs]
            for i, t in enumerate(outs):
                if t is not None:
                    self.tensors["%s/out%d" % (name, i)] = t.detach().cpu().clone()
        except (TypeError, ValueError, NotImplementedError, RuntimeError) as e:
            # a refusal IS the outcome: the host's, or the library's before it launches anything (invalid argument, unsupported shape,
            # workspace too small); anything else (a failed launch, a device error) ends the run
            if isinstance(e, RuntimeError) and not str(e).endswith(("(-1)", "(-2)", "(-4)")):
                print("row %r ended the run" % name, flush=True)
                raise
            line["exception"] = [type(e).__name__, str(e)]
        line["calls"] = list(self.rec.calls)
        self.lines.append(line)

    def write(self):
        os.makedirs(self.out_dir, exist_ok=True)
        with open(os.path.join(self.out_dir, "record.jsonl"), "w") as f:
            for line in self.lines:
                f.write(json.dumps(line, sort_keys=True) + "\n")
        torch.save(self.tensors, os.path.join(self.out_dir, "tensors.pt"))
        for l in self.lines:
            if "exception" in l:
                print("%-50s %s: %s" % (l["row"], l["exception"][0], l["exception"][1][:110]))
        print("rows %d, library calls %d, tensors %d" % (len(self.lines), sum(len(l["calls"]) for l in self.lines), len(self.tensors)))


def _rand(shape, seed, dt, dev, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dt).to(dev)


def _adj(B, n, seed, dt, dev, two_d=False):
    g = torch.Generator().manual_seed(seed)
    a = (torch.rand(B, n, n, generator=g) < 0.3).float() + torch.eye(n)
    a = (a / a.sum(-1, keepdim=True)).to(dt).to(dev)
    return a[0] if two_d else a


def _with_grads(out, gout, leaves):
    """(out, gradient of every leaf that requires grad) after out.backward(gout)."""
    out.backward(gout)
    return (out,) + tuple(t.grad for t in leaves if t is not None and t.requires_grad)


def grid(S):
    G, dev, bf, f32 = S.G, S.dev, torch.bfloat16, torch.float32

    def layer(I, O, dt, bias=True, seed=0, train=True):
        torch.manual_seed(seed)
        l = G.GraphConvolution(I, O, bias=bias).to(dt).to(dev)
        return l.train(train)

    # ---- fp32 layer
    for bx3 in ("1", "0"):
        for (B, n, I, O, two_d) in ((3, 5, 6, 4, False), (1, 5, 6, 4, True)):
            for bias in (True, False):
                for adj_grad in (False, True):
                    def run(B=B, n=n, I=I, O=O, two_d=two_d, bias=bias, adj_grad=adj_grad, bx3=bx3):
                        prev, S.gat._GEMM_BX3 = S.gat._GEMM_BX3, bx3
                        try:
                            l = layer(I, O, f32, bias)
                            x = _rand((n, I) if two_d else (B, n, I), 1, f32, dev).requires_grad_(True)
                            a = _adj(B, n, 2, f32, dev, two_d).requires_grad_(adj_grad)
                            out = l(x, a)
                            return _with_grads(out, _rand(out.shape, 3, f32, dev), [x, a, l.weight, l.bias])
                        finally:
                            S.gat._GEMM_BX3 = prev
                    S.row("f32 bx3=%s B%d n%d %d->%d 2d=%d bias=%d adjgrad=%d" % (bx3, B, n, I, O, two_d, bias, adj_grad), run)

    def max_batch(dt):
        prev, S.lib.MAX_BATCH = S.lib.MAX_BATCH, 2
        try:
            l = layer(6, 22 if dt is bf else 4, dt)
            x = _rand((5, 5, 6), 1, dt, dev).requires_grad_(True)
            out = l(x, _adj(5, 5, 2, dt, dev))
            return _with_grads(out, _rand(out.shape, 3, dt, dev), [x, l.weight, l.bias])
        finally:
            S.lib.MAX_BATCH = prev
    S.row("f32 MAX_BATCH=2 B5", lambda: max_batch(f32))
    S.row("bf16 MAX_BATCH=2 B5", lambda: max_batch(bf))

    # ---- bf16 dense layer
    for n in (5, 32, 33):
        for (I, O) in ((8, 8), (6, 22), (300, 300), (22, 328)):
            for B in (1, 3):
                for mode in ("train", "eval-nograd", "eval-grad"):
                    for adj_grad in ((False, True) if mode != "eval-nograd" else (False,)):
                        for bias in (True, False):
                            def run(n=n, I=I, O=O, B=B, mode=mode, adj_grad=adj_grad, bias=bias):
                                l = layer(I, O, bf, bias, train=(mode == "train"))
                                x = _rand((B, n, I), 1, bf, dev)
                                a = _adj(B, n, 2, bf, dev)
                                if mode == "eval-nograd":
                                    with torch.no_grad():
                                        return l(x, a), l(x, a)                    # the second call: a cache hit (planes_ready = 1)
                                x.requires_grad_(True)
                                a.requires_grad_(adj_grad)
                                out = l(x, a)
                                return _with_grads(out, _rand(out.shape, 3, bf, dev), [x, a, l.weight, l.bias])
                            S.row("bf16 n%d %d->%d B%d %s adjgrad=%d bias=%d" % (n, I, O, B, mode, adj_grad, bias), run)

    def chain(kind):
        """Two layers: the second reads what the first returned (a padded view, stride 304 for 300), or a foreign view / odd widths."""
        l1, l2 = layer(22, 300, bf, seed=1), layer(300, 6, bf, seed=2)
        x = _rand((3, 5, 22), 1, bf, dev)
        a = _adj(3, 5, 2, bf, dev)
        if kind == "padded-train":
            x.requires_grad_(True)
            h = l1(x, a)
            out = l2(h, a)
            return _with_grads(out, _rand(out.shape, 3, bf, dev), [x, l1.weight, l1.bias, l2.weight, l2.bias]) + (h,)
        if kind == "padded-nograd":
            with torch.no_grad():
                return l2.eval()(l1.eval()(x, a), a)
        buf = _rand((3, 5, 304), 4, bf, dev)
        buf[..., 300:] = float("nan")                                             # a foreign view: its pad columns must never be multiplied
        if kind == "foreign-train":
            h = buf[..., :300].requires_grad_(True)
            out = l2(h, a)
            return _with_grads(out, _rand(out.shape, 3, bf, dev), [l2.weight])
        with torch.no_grad():
            return l2.eval()(buf[..., :300], a)
    for kind in ("padded-train", "padded-nograd", "foreign-train", "foreign-nograd"):
        S.row("bf16 chain " + kind, lambda kind=kind: chain(kind))

    def odd_nograd():
        with torch.no_grad():
            return layer(7, 8, bf, train=False)(_rand((3, 5, 7), 1, bf, dev), _adj(3, 5, 2, bf, dev))
    S.row("bf16 odd I=7 contiguous nograd", odd_nograd)

    def gout_kind(kind):
        l = layer(6, 22, bf)
        x = _rand((3, 5, 6), 1, bf, dev).requires_grad_(True)
        out = l(x, _adj(3, 5, 2, bf, dev))
        if kind == "fp32":
            y = out.float()
            y.backward(_rand(out.shape, 3, f32, dev))
        else:
            out.transpose(1, 2).backward(_rand((3, 22, 5), 3, bf, dev))
        return out, x.grad, l.weight.grad, l.bias.grad
    S.row("bf16 grad_out fp32", lambda: gout_kind("fp32"))
    S.row("bf16 grad_out non-contiguous", lambda: gout_kind("nc"))

    def invalidate():
        l = layer(6, 22, bf, train=False)
        x, a = _rand((3, 5, 6), 1, bf, dev), _adj(3, 5, 2, bf, dev)
        with torch.no_grad():
            o1, o2 = l(x, a), l(x, a)
            l.weight.data.add_(0.5)
            o3 = l(x, a)                                                          # a stale hit: the version counter did not see the write
            l.invalidate_planes()
            return o1, o2, o3, l(x, a)
    S.row("bf16 eval twice, .data write, invalidate_planes", invalidate)

    def empty():
        l = layer(6, 22, bf)
        return l(torch.empty(0, 5, 6, dtype=bf, device=dev), torch.empty(0, 5, 5, dtype=bf, device=dev))
    S.row("bf16 B=0", empty)
    S.row("bf16 inconsistent shapes", lambda: layer(6, 22, bf)(_rand((3, 5, 6), 1, bf, dev), _adj(2, 5, 2, bf, dev)))
    S.row("bf16 float32 adj", lambda: layer(6, 22, bf)(_rand((3, 5, 6), 1, bf, dev), _adj(3, 5, 2, f32, dev)))

    # ---- ragged
    for sizes in ((1, 5, 32, 33), (7,)):
        for (I, O) in ((8, 8), (22, 22)):
            for vgrad in (False, True):
                def run(sizes=sizes, I=I, O=O, vgrad=vgrad):
                    l = layer(I, O, bf)
                    N = sum(sizes)
                    x = _rand((N, I), 1, bf, dev).requires_grad_(True)
                    vals = torch.cat([_adj(1, s, 2 + i, bf, dev)[0].reshape(-1) for i, s in enumerate(sizes)]).requires_grad_(vgrad)
                    rag = G.RaggedAdjacency(vals, sizes)
                    h = l(x, rag)
                    out = l(h, rag) if I == O else h                                # the second layer reads the first one's padded view
                    return _with_grads(out, _rand(out.shape, 3, bf, dev), [x, vals, l.weight, l.bias]) + (h,)
                S.row("ragged %s %d->%d vgrad=%d" % (sizes, I, O, vgrad), run)
    S.row("ragged wrong rows", lambda: layer(8, 8, bf)(_rand((5, 8), 1, bf, dev), G.RaggedAdjacency(_adj(1, 7, 2, bf, dev)[0].reshape(-1), (7,))))
    S.row("ragged float32 input", lambda: layer(8, 8, bf)(_rand((7, 8), 1, f32, dev), G.RaggedAdjacency(_adj(1, 7, 2, bf, dev)[0].reshape(-1), (7,))))

    # ---- gcn_stack
    def stack(B, n, I, D, nl, train, bias=True, frozen=None, padded_x=False, adj_grad=False, nc_x=False, twice=False, env=None, ragged=False,
              x_grad=True):
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            G.invalidate_stack_planes()
            layers = [layer(I if i == 0 else D, D, bf, bias, seed=10 + i, train=train) for i in range(nl)]
            if frozen is not None:
                for p in layers[frozen].parameters():
                    p.requires_grad_(False)
            if ragged:
                a = G.RaggedAdjacency(torch.cat([_adj(1, n, 2 + b, bf, dev)[0].reshape(-1) for b in range(B)]), (n,) * B)
                x = _rand((B * n, I), 1, bf, dev)
            else:
                a = _adj(B, n, 2, bf, dev).requires_grad_(adj_grad)
                x = _rand((B, n, I), 1, bf, dev)
            if padded_x:
                with torch.no_grad():
                    x = layer(I, I, bf, seed=9, train=False)(x, a)                  # the padded view a previous layer returned
            if nc_x:
                x = _rand((B, I, n), 1, bf, dev).transpose(1, 2)
            if not train:
                with torch.no_grad():
                    out = G.gcn_stack(x, a, layers)
                    return (out, G.gcn_stack(x, a, layers)) if twice else out
            x = x.detach().requires_grad_(x_grad)
            out = G.gcn_stack(x, a, layers)
            leaves = [x, None if ragged else a] + [p for l in layers for p in l.parameters()]
            return _with_grads(out, _rand(out.shape, 3, bf, dev), leaves)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    # the shapes of tests/test_prop_gpu.py's two stack tests with B <= 9 (n = 31 falls back; I = 37 falls back in inference and is packed in training)
    for (B, n, I, D, nl) in ((9, 32, 300, 300, 3), (5, 32, 40, 136, 2), (7, 8, 300, 64, 4), (3, 12, 22, 320, 3), (6, 31, 300, 300, 3), (6, 28, 37, 300, 2)):
        for train in (False, True):
            S.row("stack B%d n%d %d->%d L%d train=%d" % (B, n, I, D, nl, train), lambda B=B, n=n, I=I, D=D, nl=nl, train=train: stack(B, n, I, D, nl, train, twice=not train))
    S.row("stack no bias", lambda: stack(2, 8, 22, 64, 2, True, bias=False))
    S.row("stack no bias infer", lambda: stack(2, 8, 22, 64, 2, False, bias=False))
    S.row("stack frozen middle, padded x, B2", lambda: stack(2, 8, 300, 300, 3, True, frozen=1, padded_x=True))
    S.row("stack padded x infer", lambda: stack(2, 8, 300, 300, 3, False, padded_x=True))
    S.row("stack x without grad", lambda: stack(2, 8, 22, 64, 2, True, x_grad=False))
    S.row("stack fallback: one layer", lambda: stack(2, 8, 8, 8, 1, True))
    S.row("stack fallback: n=31 train", lambda: stack(2, 31, 8, 8, 2, True))
    S.row("stack fallback: n=6 infer", lambda: stack(2, 6, 8, 8, 2, False))
    S.row("stack fallback: D=324", lambda: stack(2, 8, 324, 324, 2, False))
    S.row("stack fallback: I=324 train", lambda: stack(2, 8, 324, 8, 2, True))
    S.row("stack fallback: adj requires grad", lambda: stack(2, 8, 8, 8, 2, True, adj_grad=True))
    S.row("stack fallback: ragged", lambda: stack(2, 8, 8, 8, 2, True, ragged=True))
    S.row("stack fallback: RECON_GCN_STACK=0", lambda: stack(2, 8, 8, 8, 2, False, env={"RECON_GCN_STACK": "0"}))
    S.row("stack fallback: RECON_GCN_STACK_TRAIN=0", lambda: stack(2, 8, 8, 8, 2, True, env={"RECON_GCN_STACK_TRAIN": "0"}))
    S.row("stack fallback: non-contiguous x infer", lambda: stack(2, 8, 8, 8, 2, False, nc_x=True))
    # in_features > 384 passes the host's test in inference; recon_gcn_b16_stack_fwd answers RECON_ERR_UNSUPPORTED (-2: its LDS image) and the loop runs
    S.row("stack library answers -2: I=392 infer", lambda: stack(2, 8, 392, 8, 2, False))


def compare(a, b):
    la, lb = [open(os.path.join(d, "record.jsonl")).read().splitlines() for d in (a, b)]
    bad = 0
    if len(la) != len(lb):
        print("records differ in length: %d against %d" % (len(la), len(lb)))
        bad += 1
    for x, y in zip(la, lb):
        if x != y:
            bad += 1
            print("record differs at row %r" % json.loads(x)["row"])
    ta, tb = torch.load(os.path.join(a, "tensors.pt")), torch.load(os.path.join(b, "tensors.pt"))
    if sorted(ta) != sorted(tb):
        print("tensor names differ")
        bad += 1
    nd = 0
    for k in sorted(set(ta) & set(tb)):
        u, v = ta[k], tb[k]
        same = u.shape == v.shape and u.dtype == v.dtype and torch.equal(u.contiguous().view(torch.uint8), v.contiguous().view(torch.uint8))
        if not same:
            nd += 1
            d = (u.double() - v.double()).abs().max().item() if u.shape == v.shape else float("nan")
            print("tensor differs: %s (max abs difference %.3e, max abs value %.3e)" % (k, d, u.double().abs().max().item()))
    print("%d record lines, %d differ; %d tensors, %d differ" % (len(la), bad, len(ta), nd))
    return 1 if bad or nd else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--impl")
    ap.add_argument("--compare", nargs=2)
    o = ap.parse_args()
    if o.compare:
        sys.exit(compare(*o.compare))
    S = Session(o.out, o.impl)
    grid(S)
    S.write()
