import os, sys, json
_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, _ROOT); sys.path.insert(0, os.path.join(_ROOT, 'tools'))
import torch
torch.autograd.set_multithreading_enabled(False)
import secondary
print(json.dumps(secondary.powerlaw_mixed_stack_bf16(iters=20)))
