"""Host time of GraphConvolution x 3 at cfg 3a (no synchronisation inside the timed region; the queue is drained every 20 iterations).

    --path stack-train     one gcn_stack() training iteration: forward, backward (the default)
    --path layers-nograd   the eval()-mode layer loop under torch.no_grad(): the path that skips the autograd.Function machinery
    --no-profile           the two figures only, as one JSON line behind the text"""
import argparse, json, os, sys, time, cProfile, pstats
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from recon_amd.gcn_layers import GraphConvolution, gcn_stack
ap = argparse.ArgumentParser()
ap.add_argument("--path", choices=("stack-train", "layers-nograd"), default="stack-train")
ap.add_argument("--no-profile", action="store_true")
ap.add_argument("--iters", type=int, default=200)
opt = ap.parse_args()
torch.autograd.set_multithreading_enabled(False)
dv = torch.device("cuda:0"); dt = torch.bfloat16
B, n, D, hops = 1024, 32, 300, 3
g = torch.Generator().manual_seed(0)
x = torch.randn(B, n, D, generator=g).to(dt).to(dv).requires_grad_(True)
adj = (torch.rand(B, n, n, generator=g) < 0.15).float() + torch.eye(n)
adj = (adj / adj.sum(-1, keepdim=True)).to(dt).to(dv)
layers = [GraphConvolution(D, D).to(dt).to(dv) for _ in range(hops)]
G = torch.randn(B, n, D, generator=g).to(dt).to(dv)

def it_train():
    for l in layers:
        l.weight.grad = None; l.bias.grad = None
    x.grad = None
    t0 = time.perf_counter()
    y = gcn_stack(x, adj, layers)
    t1 = time.perf_counter()
    y.backward(G)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1

def it_nograd():
    t0 = time.perf_counter()
    with torch.no_grad():
        h = x
        for l in layers:
            h = l(h, adj)
    return time.perf_counter() - t0, 0.0

it = it_train if opt.path == "stack-train" else it_nograd
if opt.path == "layers-nograd":
    for l in layers:
        l.eval()
for _ in range(5): it()
torch.cuda.synchronize()
f = b = 0.0; N = opt.iters
for i in range(N):
    a, c = it(); f += a; b += c
    if i % 20 == 19: torch.cuda.synchronize()
print("host us per iteration: forward %.1f backward %.1f" % (f / N * 1e6, b / N * 1e6))
print(json.dumps({"probe": "gcn_host_time", "path": opt.path, "iters": N, "forward_us": f / N * 1e6, "backward_us": b / N * 1e6}))
if not opt.no_profile:
    pr = cProfile.Profile(); pr.enable()
    for i in range(100):
        it()
        if i % 20 == 19: torch.cuda.synchronize()
    pr.disable()
    pstats.Stats(pr).sort_stats("tottime").print_stats(14)
