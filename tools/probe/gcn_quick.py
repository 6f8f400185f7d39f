import os, sys, json
_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, _ROOT); sys.path.insert(0, os.path.join(_ROOT, 'tools'))
import torch
torch.autograd.set_multithreading_enabled(False)      # one device: the engine's worker thread only adds a hand-over (as bench.py does)
import secondary
print(json.dumps(secondary.gcn_bf16(iters=20)))
