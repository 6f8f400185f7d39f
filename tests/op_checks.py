"""The acceptance rules of the fused encoder ops (char-CNN, its masked form, line LSTM, pair LSTM, translation residuals, transition
projections), said once: the error band, the wiring rule's call counter, bitwise equality, the "materialises nothing" memory
measurement, the whole-model fixtures through an op, and the header / `_lib.SYMBOLS` check.  tests/test_op_checks_cpu.py shows on the
CPU that they bite.  Not a test module and not a conftest: the op test files import from it."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden


def dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------- the band
# Errors are relative to max |fp64 oracle|.  The stock fp32 chain's own error on the same inputs, e_chain, is measured in the test and
# the op has to stay within 4 e_chain (4x for another summation order), but is never asked for less than 2^-20 (the bound of
# test_sgemm_hx2) and never allowed more than 2e-5 (the figure README.md gives).
def bound(e_chain):
    return min(max(4 * e_chain, 2.0 ** -20), 2e-5)


def rel_err(got, ref):
    return ((got.detach().double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def band_failures(names, got, chain, ref, label):
    """The outputs of `got` outside the band that `chain`'s own error sets, as (name, e_op, e_chain); prints every figure.  A None in
    `ref` (an output the case does not have) requires a None in `got`."""
    bad = []
    for what, f, c, r in zip(names, got, chain, ref):
        assert (f is None) == (r is None), (what, "None against a tensor")
        if r is None:
            continue
        assert f.shape == r.shape, (what, f.shape, r.shape)
        e_f, e_c = rel_err(f, r), rel_err(c, r)
        print("%s %s: op %.3e chain %.3e bound %.3e ratio %.3f" % (label, what, e_f, e_c, bound(e_c), e_f / bound(e_c)))
        if not e_f <= bound(e_c):
            bad.append((what, e_f, e_c))
    return bad


def close(actual, desired, atol=1e-4, rel_to_max=1e-4, what=""):
    actual = actual.detach().cpu().numpy() if torch.is_tensor(actual) else actual
    desired = desired.detach().cpu().numpy() if torch.is_tensor(desired) else desired
    tol = atol + rel_to_max * (np.abs(desired).max() if desired.size else 0.0)
    err = np.abs(actual - desired).max() if desired.size else 0.0
    assert np.isfinite(actual).all(), what + ": non-finite values"
    assert err <= tol, "%s: max abs err %.3e > tol %.3e" % (what, err, tol)


def same(a, b):
    """Two lists agree bit for bit, a None only against a None."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------- the wiring rule
def calls_of(monkeypatch, owner, name):
    """Wraps `owner.name` for the rest of the test: every call appends to the returned list and passes through."""
    calls = []
    real = getattr(owner, name)

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    is_apply = isinstance(owner, type) and issubclass(owner, torch.autograd.Function)
    monkeypatch.setattr(owner, name, staticmethod(counted) if is_apply else counted)
    return calls


# ------------------------------------------------------------------------------------------------------------- memory
def rounded(nbytes):
    return (nbytes + 511) // 512 * 512       # torch.cuda.memory_allocated counts whole 512-byte blocks


def peak_bytes(fn):
    """(peak of torch.cuda.max_memory_allocated above what was allocated before, fn()'s result) of the second of two calls."""
    out = fn()                                # warm-up: library load, allocator pools
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


# ------------------------------------------------------------------------------------------------------------- the fixtures' models
def state_dict_of(g):
    return {k[3:]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith("sd.")}


def gpgnn_fixture(name):
    """(model, fixture, model -> logits, name) of a fixture written from the reference's GPGNN."""
    from recon_amd.gpgnn import GPGNN
    g = load_golden(name)
    p = {"max_num_nodes": int(g["n"]), "embedding_dim": int(g["d"]), "layer_number": int(g["L"]), "projection_style": str(g["style"]),
         "non-linear1": "relu", "non-linear": "tanh", "dropout1": 0.0, "position_emb": 3, "units1": 4, "rnn1_layers": 1,
         "bidirectional": 1, "batch_size": int(g["B"])}
    m = GPGNN(p, g["emb"], max_sent_len=4, n_out=3)
    m.load_state_dict(state_dict_of(g), strict=False)
    return m, g, lambda m: m(torch.from_numpy(g["sent"]).to(dev()), torch.from_numpy(g["mark"]).to(dev()), None), name


def _eac_fixture(cls, params, name, extra):
    g = load_golden(name)
    m = cls(dict(params), g["emb"], max_sent_len=4, n_out=3, char_vocab=list(range(int(g["n_chars"]))))
    m.load_state_dict(state_dict_of(g), strict=False)
    t = lambda k: torch.from_numpy(g[k]).to(dev())
    return m, g, lambda m: m(t("sent"), t("mark"), None, None, None, t("ctx_words"), t("ctx_chars"), t("ctx_mask"), t("pos"), int(g["max_occ"]),
                             *[t(k) for k in extra]), name


def eac_fixture():
    from recon_amd.gpgnn import RECON_EAC
    from tests.test_host_cpu import EAC_P
    return _eac_fixture(RECON_EAC, EAC_P, "eac1_untied", ())


def kggat_fixture():
    from recon_amd.gpgnn import RECON_EAC_KGGAT
    from tests.test_host_cpu import KGGAT_P
    return _eac_fixture(RECON_EAC_KGGAT, KGGAT_P, "kggat1_untied", ("gat",))


def pinned(m, g, out_of, what, monkeypatch, switch, calls, forbidden, required):
    """A reference fixture through an op with the stock module made to fail: `switch` is the model's attribute that turns the op on,
    `calls` the op's call counter, `forbidden(m)` the modules whose forward must not run with the message of the failure, and
    `required` the gradient keys the fixture must hold (an entry ending in "." is a prefix)."""
    setattr(m, switch, True)
    m.train().to(dev())
    modules, message = forbidden(m)
    for mod in modules:
        monkeypatch.setattr(mod, "forward", lambda *a, **k: pytest.fail(message))
    out = out_of(m)
    assert len(calls) == 1
    close(out, g["out"], atol=1e-4, what=what + " logits")
    (out * torch.from_numpy(g["G"]).to(dev())).sum().backward()
    seen = 0
    for k, v in m.named_parameters():
        if "g." + k in g:
            close(v.grad, g["g." + k], atol=1e-4, rel_to_max=1e-4, what=what + " grad " + k)
            seen += 1
    assert seen == sum(k.startswith("g.") for k in g)
    for key in required:
        assert any(k.startswith(key) for k in g) if key.endswith(".") else key in g, key


# ------------------------------------------------------------------------------------------------------------- the C ABI's entries
def entries_declared_and_bound(names, cites):
    """include/recon_hip.h declares every entry outside a comment, `_lib.SYMBOLS` binds it, and the comment in front of it cites its
    lines of the reference."""
    from recon_amd import _lib
    raw = open(os.path.join(ROOT, "include", "recon_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    bound_names = {name for name, _, _ in _lib.SYMBOLS}
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in bound_names, name
        comment = raw[:raw.index(name + "(")].rsplit("/*", 1)[1]
        assert cites in comment, name
