"""CPU-side checks of the optimizer entry points (csrc/optim.hip, recon_amd/optim.py): declared, exported and bound; the argument checks
that return before any launch; the size queries; and what the Python classes refuse at construction."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

OPTIM_SYMBOLS = ("recon_optim_sgd", "recon_optim_adam", "recon_optim_grad_sumsq", "recon_optim_workspace_bytes", "recon_optim_max_segments",
                 "recon_optim_chunk_elems")


def test_optim_symbols_declared_exported_bound():
    from recon_amd import _lib
    header = open(os.path.join(ROOT, "include", "recon_hip.h")).read()
    h = ctypes.CDLL(_lib.LIB_PATH)
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in OPTIM_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(h, name), name
        assert name in bound, name
    assert _lib.lib().recon_version() == 2
    assert "optim.hip" in open(os.path.join(ROOT, "recon_amd", "csrc", "Makefile")).read()


def test_optim_size_queries():
    from recon_amd import _lib
    L = _lib.lib()
    assert L.recon_optim_max_segments() >= 16
    ch = L.recon_optim_chunk_elems()
    assert ch > 0 and ch % 4 == 0
    # 16 bytes of results + one 8-byte word per workgroup; a segment of n elements has ceil(n / ch) workgroups
    for sizes in ([1], [ch], [ch + 1, 3, 2 * ch - 1], [5] * 70):
        groups = sum(-(-n // ch) for n in sizes)
        assert L.recon_optim_workspace_bytes(sum(sizes), len(sizes)) >= 16 + 8 * groups
    assert L.recon_optim_workspace_bytes(0, 0) >= 16


def test_optim_argument_checks_return_before_a_launch():
    from recon_amd import _lib
    L = _lib.lib()
    fake = 16                                                                # never dereferenced: every call below returns before a launch
    ptrs = (ctypes.c_void_p * 3)(fake, fake, fake)
    empty, some, negative = (ctypes.c_int64 * 3)(0, 0, 0), (ctypes.c_int64 * 3)(4, 0, 9), (ctypes.c_int64 * 3)(4, -1, 9)
    hole = (ctypes.c_void_p * 3)(fake, None, fake)                           # a null segment pointer: only matters where there are elements
    sgd = lambda P, G, N, n: L.recon_optim_sgd(P, G, N, n, 0.1, 0.0, None, None)
    adam = lambda P, G, M, V, N, n: L.recon_optim_adam(P, G, M, V, N, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, None, None)
    sumsq = lambda G, N, n, ws=fake: L.recon_optim_grad_sumsq(G, N, n, 1.0, ws, 1 << 20, None)
    assert sgd(ptrs, ptrs, some, -1) == -1 and adam(ptrs, ptrs, ptrs, ptrs, some, -1) == -1 and sumsq(ptrs, some, -1) == -1
    assert sgd(None, ptrs, some, 3) == -1 and sgd(ptrs, None, some, 3) == -1 and sgd(ptrs, ptrs, None, 3) == -1
    for k in range(4):
        args = [ptrs] * 4
        args[k] = None
        assert adam(*args, some, 3) == -1
    assert sumsq(None, some, 3) == -1 and sumsq(ptrs, None, 3) == -1 and sumsq(ptrs, some, 3, ws=None) == -1
    assert sgd(ptrs, ptrs, negative, 3) == -1 and adam(ptrs, ptrs, ptrs, ptrs, negative, 3) == -1 and sumsq(ptrs, negative, 3) == -1
    assert sgd(ptrs, hole, (ctypes.c_int64 * 3)(4, 2, 9), 3) == -1 and sumsq(hole, (ctypes.c_int64 * 3)(4, 2, 9), 3) == -1
    assert sgd(ptrs, ptrs, some, 0) == 0 and adam(ptrs, ptrs, ptrs, ptrs, some, 0) == 0 and sumsq(ptrs, some, 0) == 0
    assert sgd(None, None, None, 0) == 0 and sumsq(None, None, 0, ws=None) == 0
    assert sgd(ptrs, ptrs, empty, 3) == 0 and adam(ptrs, ptrs, ptrs, ptrs, empty, 3) == 0 and sumsq(ptrs, empty, 3) == 0
    assert sgd(hole, hole, empty, 3) == 0
    # Adam's bias corrections are 1 - beta^t with t >= 1: positive
    assert L.recon_optim_adam(ptrs, ptrs, ptrs, ptrs, some, 3, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.001, None, None) == -1
    assert L.recon_optim_grad_sumsq(ptrs, some, 3, 1.0, fake, 16, None) == -4     # workspace below recon_optim_workspace_bytes()


def test_optim_refuses_cpu_parameters_and_unsupported_options():
    from recon_amd.optim import SGD, Adam
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        SGD([p], lr=0.1)
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        Adam([p])
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        Adam([{"params": [p], "lr": 0.1}], weight_decay=1e-5, max_grad_norm=1.0)
    for kw in ({"momentum": 0.9}, {"nesterov": True}, {"dampening": 0.1}, {"maximize": True}):
        with pytest.raises(TypeError, match="does not implement"):
            SGD([p], lr=0.1, **kw)
    for kw in ({"amsgrad": True}, {"maximize": True}, {"decoupled_weight_decay": True}):
        with pytest.raises(TypeError, match="does not implement"):
            Adam([p], **kw)
    for make in (lambda: SGD([p], lr=-1.0), lambda: SGD([p], lr=0.1, weight_decay=-1.0), lambda: Adam([p], lr=-1.0), lambda: Adam([p], eps=-1.0),
                 lambda: Adam([p], betas=(1.0, 0.999)), lambda: Adam([p], weight_decay=-1.0), lambda: SGD([p], lr=0.1, max_grad_norm=0.0),
                 lambda: Adam([p], max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            make()
    assert issubclass(SGD, torch.optim.Optimizer) and issubclass(Adam, torch.optim.Optimizer)
    for cls in (SGD, Adam):                                                  # the base class's, not overridden
        for name in ("zero_grad", "add_param_group", "state_dict", "load_state_dict"):
            assert getattr(cls, name) is getattr(torch.optim.Optimizer, name), (cls, name)
