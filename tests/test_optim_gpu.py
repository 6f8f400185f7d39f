"""recon_amd.optim.SGD / Adam (csrc/optim.hip) on the device: parity with torch.optim in fp64 (the oracle) and in fp32 (the reference
arithmetic) over a parameter set that takes every path of the kernels, skipped parameters, bitwise determinism of the clipped step, the
absence of torch ops in the steady state, state_dict interchange with torch.optim.Adam, and the reference's own recorded training steps."""
import copy
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.from_numpy
MAGNITUDES = (1e-3, 1e-2, 1e-1, 1.0, 10.0)          # gradient magnitude of step k: MAGNITUDES[k % 5]
STEPS = 20
CLIP = 0.5


@functools.lru_cache(None)
def layout():
    """(shapes, index of the 4-byte-aligned view, of the frozen parameter, of the one without a gradient on odd steps).  CH = the
    kernels' chunk: one element, a tail below one 16-byte access, several rows, exactly a chunk, a chunk and one, two chunks and an odd
    tail; then (2,) parameters until an even step has one segment more than a launch takes."""
    from recon_amd import _lib
    L = _lib.lib()
    ch, max_segs = L.recon_optim_chunk_elems(), L.recon_optim_max_segments()
    shapes = [(1,), (3,), (5, 7), (ch,), (ch + 1,), (2, 2 * ch - 1), (6, 11), (4,), (9,)]
    view, frozen, sometimes = 6, 7, 8
    shapes += [(2,)] * (max_segs + 1 - (len(shapes) - 1))
    assert len(shapes) - 1 == max_segs + 1
    return tuple(shapes), view, frozen, sometimes


@functools.lru_cache(None)
def inputs():
    """Initial values and the gradients of every step (fp32, CPU), made once; gradient None: the parameter has none at that step."""
    shapes, _, frozen, sometimes = layout()
    g = torch.Generator().manual_seed(1234)
    init = [torch.randn(s, generator=g) * 0.5 for s in shapes]
    grads = []
    for k in range(STEPS):
        row = []
        for i, s in enumerate(shapes):
            t = torch.randn(s, generator=g) * MAGNITUDES[k % 5]
            row.append(None if i == frozen or (i == sometimes and k % 2 == 1) else t)
        grads.append(row)
    return init, grads


def cpu_params(dtype):
    shapes, _, frozen, _ = layout()
    return [torch.nn.Parameter(v.to(dtype).clone(), requires_grad=(i != frozen)) for i, v in enumerate(inputs()[0])]


def device_params():
    """The same values on the device; parameter `view` starts one float into a larger buffer: its address is 4-byte aligned only."""
    shapes, view, frozen, _ = layout()
    out = []
    for i, v in enumerate(inputs()[0]):
        if i == view:
            buf = torch.zeros(v.numel() + 8, device=DEV)
            t = buf[1:1 + v.numel()].view(v.shape)
            t.copy_(v)
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
            out.append(t.requires_grad_(True))
        else:
            out.append(torch.nn.Parameter(v.to(DEV), requires_grad=(i != frozen)))
    return out


def snapshot(params, opt, adam):
    snap = {"p": [p.detach().cpu().double() for p in params]}
    if adam:
        for key in ("exp_avg", "exp_avg_sq"):
            snap[key] = [opt.state[p][key].detach().cpu().double() if key in opt.state.get(p, {}) else None for p in params]
        snap["step"] = [float(opt.state[p]["step"]) if "step" in opt.state.get(p, {}) else 0.0 for p in params]
    return snap


def make_torch(kind, params, wd, **kw):
    if kind == "sgd":
        return torch.optim.SGD(params, lr=1e-2, weight_decay=wd, **kw)
    return torch.optim.Adam(params, lr=1e-3, weight_decay=wd, **kw)


def make_recon(kind, params, wd, clip):
    from recon_amd.optim import SGD, Adam
    if kind == "sgd":
        return SGD(params, lr=1e-2, weight_decay=wd, max_grad_norm=clip)
    return Adam(params, lr=1e-3, weight_decay=wd, max_grad_norm=clip)


@functools.lru_cache(None)
def reference(kind, wd, clip, dtype):
    """torch.optim on the CPU in `dtype` over all STEPS steps (clip_grad_norm_ in front where the case clips): snapshots after 1 and after
    STEPS steps, and the fp64 gradient norms."""
    params = cpu_params(dtype)
    opt = make_torch(kind, params, wd, foreach=False)
    snaps, norms = {}, []
    for k, row in enumerate(inputs()[1]):
        for p, g in zip(params, row):
            p.grad = None if g is None else g.to(dtype).clone()
        if clip is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, clip, foreach=False)))
        opt.step()
        if k + 1 in (1, STEPS):
            snaps[k + 1] = snapshot(params, opt, kind == "adam")
    return snaps, norms


def hand_over(params, row, k, bucket):
    """The gradients of one step, three ways in turn: fresh tensors; views into a FlatGradBucket after pack() (arbitrary float offsets);
    non-contiguous tensors set by hand."""
    way = k % 3
    for p, g in zip(params, row):
        if g is None:
            p.grad = None
        elif way == 2:
            if g.dim() == 2:
                ng = g.t().contiguous().to(DEV).t()
            else:
                ng = torch.zeros(2 * g.numel(), device=DEV)[::2]
                ng.copy_(g)
            assert not ng.is_contiguous() or g.numel() == 1
            p.grad = ng
        else:
            p.grad = g.to(DEV)
    if way == 1:
        bucket.pack()
        for p, g in zip(params, row):
            if g is None:
                p.grad = None                                               # pack() gave it zeros: this step it has NO gradient
        assert any(p.grad is not None and p.grad.data_ptr() % 16 for p in params)


def run_device(kind, wd, clip, steps=STEPS, snaps_at=(1, STEPS)):
    from recon_amd.dist import FlatGradBucket
    params = device_params()
    opt = make_recon(kind, params, wd, clip)
    bucket = FlatGradBucket(params)
    snaps, norms = {}, []
    for k, row in enumerate(inputs()[1][:steps]):
        hand_over(params, row, k, bucket)
        opt.step()
        if clip is not None:
            norms.append(opt.last_grad_norm.item())
        if k + 1 in snaps_at:
            snaps[k + 1] = snapshot(params, opt, kind == "adam")
    return params, opt, snaps, norms


def check_bound(dev, f64, f32, what):
    """Per tensor: max|dev - f64| <= 2 max|torch32 - f64| + 2^-22 max|f64|.  Returns the largest observed ratio."""
    worst = 0.0
    for key in dev:
        if key == "step":
            assert dev[key] == f64[key] == f32[key], (what, key)
            continue
        for i, (a, b, c) in enumerate(zip(dev[key], f64[key], f32[key])):
            if b is None:
                assert a is None and c is None, (what, key, i)
                continue
            assert a is not None and torch.isfinite(a).all(), (what, key, i)
            err, ref = (a - b).abs().max().item(), (c - b).abs().max().item()
            bound = 2.0 * ref + 2.0 ** -22 * b.abs().max().item()
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else float("inf")))
            assert err <= bound, "%s: %s[%d] shape %s: |dev - f64| = %.3e > bound %.3e (torch32 at %.3e)" % (what, key, i, tuple(a.shape), err, bound, ref)
    return worst


@pytest.mark.parametrize("clip", [None, CLIP])
@pytest.mark.parametrize("kind,wd", [("sgd", 0.0), ("sgd", 1e-4), ("adam", 0.0), ("adam", 1e-5)])
def test_optim_parity_with_fp64_and_torch(kind, wd, clip):
    ref64, _ = reference(kind, wd, clip, torch.float64)
    ref32, _ = reference(kind, wd, clip, torch.float32)
    _, _, snaps, _ = run_device(kind, wd, clip)
    for n in (1, STEPS):
        worst = check_bound(snaps[n], ref64[n], ref32[n], "%s wd=%g clip=%s after %d steps" % (kind, wd, clip, n))
        print("optim parity %s wd=%g clip=%s steps=%d: worst error / bound = %.3f" % (kind, wd, clip, n, worst))


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_optim_skipped_parameters_are_untouched(kind):
    _, _, frozen, sometimes = layout()
    before = [v.clone() for v in inputs()[0]]
    params, opt, snaps, _ = run_device(kind, 1e-4, CLIP, steps=2, snaps_at=(1, 2))
    assert torch.equal(params[frozen].detach().cpu(), before[frozen])                      # bit-identical: never written
    assert torch.equal(snaps[1]["p"][frozen], snaps[2]["p"][frozen])
    assert not torch.equal(snaps[1]["p"][sometimes].float(), before[sometimes])            # step 0 had a gradient ...
    assert torch.equal(snaps[1]["p"][sometimes], snaps[2]["p"][sometimes])                 # ... step 1 had none
    assert not torch.equal(snaps[1]["p"][0], snaps[2]["p"][0])
    if kind == "adam":
        assert snaps[2]["step"][sometimes] == 1.0 and snaps[2]["step"][0] == 2.0 and snaps[2]["step"][frozen] == 0.0
        assert len(opt.state[params[frozen]]) == 0
        assert torch.equal(snaps[1]["exp_avg"][sometimes], snaps[2]["exp_avg"][sometimes])
        assert torch.equal(snaps[1]["exp_avg_sq"][sometimes], snaps[2]["exp_avg_sq"][sometimes])
        st = opt.state[params[0]]["step"]
        assert st.device.type == "cpu" and st.dim() == 0 and st.dtype == torch.float32     # torch.optim.Adam's representation


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_optim_clipped_step_is_deterministic(kind):
    runs = [run_device(kind, 1e-5, CLIP, steps=5, snaps_at=(5,)) for _ in range(2)]
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a.detach(), b.detach())
    assert runs[0][3] == runs[1][3]
    for k, norm in enumerate(runs[0][3]):
        n64 = float(np.sqrt(sum(float((g.double() ** 2).sum()) for g in inputs()[1][k] if g is not None)))
        ulps = abs(norm - n64) / float(np.spacing(np.float32(n64)))
        print("optim %s step %d: last_grad_norm %.9g, fp64 %.17g, %.2f ulp" % (kind, k, norm, n64, ulps))
        assert ulps <= 4.0, (k, norm, n64)


@pytest.mark.parametrize("clip", [None, CLIP])
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_optim_steady_state_issues_no_torch_op(kind, clip):
    params = device_params()
    opt = make_recon(kind, params, 1e-5, clip)
    rows = [[None if g is None else g.to(DEV) for g in row] for row in inputs()[1][:6]]
    addresses = None
    for k, row in enumerate(rows):
        for p, g in zip(params, row):
            p.grad = g
        if k < 2:
            opt.step()
        else:
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
                opt.step()
            ops = sorted({ev.name for ev in prof.events() if ev.name.startswith("aten::")})
            assert ops == [], "step %d recorded %s" % (k, ops)
        now = [p.data_ptr() for p in params]
        if kind == "adam":
            now += [opt.state[p][key].data_ptr() for p in params if opt.state.get(p) for key in ("exp_avg", "exp_avg_sq")]
            now += [id(opt.state[p]["step"]) for p in params if opt.state.get(p)]
        assert addresses is None or now == addresses, "step %d moved a parameter or its state" % k
        addresses = now
    torch.cuda.synchronize()
    if kind == "adam":
        assert float(opt.state[params[0]]["step"]) == 6.0


# ---- interchange with torch.optim.Adam ------------------------------------------------------------------------------------------------
N_SMALL = 7            # the first parameters of the set (every one has a gradient at every step), the 4-byte-aligned view among them
WD = 1e-5


def small_device_params():
    return device_params()[:N_SMALL]


@functools.lru_cache(None)
def small_reference(dtype, scheduled):
    params = cpu_params(dtype)[:N_SMALL]
    opt = torch.optim.Adam(params, lr=1e-2, weight_decay=WD, foreach=False)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5) if scheduled else None
    for row in inputs()[1][:6]:
        for p, g in zip(params, row):
            p.grad = g.to(dtype).clone()
        opt.step()
        if sched is not None:
            sched.step()
    return snapshot(params, opt, True)


def drive(opt, params, rows, sched=None):
    for row in rows:
        for p, g in zip(params, row):
            p.grad = g.to(DEV)
        opt.step()
        if sched is not None:
            sched.step()


@pytest.mark.parametrize("direction", ["torch_to_recon", "recon_to_torch"])
def test_optim_adam_state_interchanges_with_torch(direction):
    from recon_amd.optim import Adam
    rows = inputs()[1][:6]
    first, second = small_device_params(), None
    mk_torch = lambda ps: torch.optim.Adam(ps, lr=1e-2, weight_decay=WD)
    mk_recon = lambda ps: Adam(ps, lr=1e-2, weight_decay=WD)
    a = (mk_torch if direction == "torch_to_recon" else mk_recon)(first)
    drive(a, first, rows[:3])
    second = [p.detach().clone().requires_grad_(True) for p in first]
    b = (mk_recon if direction == "torch_to_recon" else mk_torch)(second)
    b.load_state_dict(copy.deepcopy(a.state_dict()))
    drive(b, second, rows[3:])
    drive(a, first, rows[3:])                                               # the writer goes on as well: "on both"
    ref64, ref32 = small_reference(torch.float64, False), small_reference(torch.float32, False)
    for opt, params, who in ((b, second, "loader"), (a, first, "writer")):
        worst = check_bound(snapshot(params, opt, True), ref64, ref32, "%s, %s" % (direction, who))
        print("optim interchange %s %s: worst error / bound = %.3f" % (direction, who, worst))
    assert all(float(b.state[p]["step"]) == 6.0 for p in second)


def test_optim_adam_follows_a_scheduler_like_torch():
    from recon_amd.optim import Adam
    rows = inputs()[1][:6]
    ref64, ref32 = small_reference(torch.float64, True), small_reference(torch.float32, True)
    for name, make in (("recon", lambda ps: Adam(ps, lr=1e-2, weight_decay=WD)), ("torch", lambda ps: torch.optim.Adam(ps, lr=1e-2, weight_decay=WD))):
        params = small_device_params()
        opt = make(params)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
        drive(opt, params, rows, sched)
        assert abs(opt.param_groups[0]["lr"] - 1e-2 / 8) < 1e-12
        worst = check_bound(snapshot(params, opt, True), ref64, ref32, "StepLR, " + name)
        print("optim StepLR %s: worst error / bound = %.3f" % (name, worst))


# ---- the reference's own recorded steps -----------------------------------------------------------------------------------------------
def close(actual, desired, atol=1e-4, rel_to_max=1e-4, what=""):
    actual = actual.detach().cpu().numpy() if torch.is_tensor(actual) else actual
    desired = desired.detach().cpu().numpy() if torch.is_tensor(desired) else desired
    tol = atol + rel_to_max * (np.abs(desired).max() if desired.size else 0.0)
    err = np.abs(actual - desired).max() if desired.size else 0.0
    assert np.isfinite(actual).all(), what + ": non-finite values"
    assert err <= tol, "%s: max abs err %.3e > tol %.3e" % (what, err, tol)


def test_optim_sgd_spkbgat_three_iterations_golden(monkeypatch):
    """Stage A as the reference ran it (GAT/main.py:478-525: SpKBGATModified in train(), three iterations of forward -> batch_gat_loss
    -> backward -> SGD(lr = 1e-3) on three batches, the recorded dropout factors replayed), with recon_amd.optim.SGD doing the update:
    the reference's losses, final parameters and the three updates themselves."""
    from recon_amd import models
    from recon_amd.models import SpKBGATModified
    from recon_amd.losses import batch_gat_loss
    from recon_amd.optim import SGD
    monkeypatch.setattr(models, "KEEP_PRUNED_POSITIONS", True)
    g = load_golden("spkbgat3_train")
    d = DEV
    H, nhid, ratio = int(g["nheads"]), int(g["nhid"]), int(g["ratio"])
    sd0 = {k[3:]: T(g[k]) for k in g if k.startswith("p0.")}
    m = SpKBGATModified(sd0["entity_embeddings"].clone(), sd0["relation_embeddings"].clone(), [nhid, nhid * H], [nhid * H, nhid * H],
                        float(g["p_drop"]), float(g["alpha"]), [H, H], None)
    m.load_state_dict(sd0, strict=True)
    m = m.to(d).train()
    sg = m.sparse_gat_1
    opt = SGD(m.parameters(), lr=float(g["lr"]))
    loss_fn = torch.nn.MarginRankingLoss(margin=float(g["margin"]))
    kept = lambda mk: mk if m._pruned_pos is None else mk.reshape(-1)[m._pruned_pos]       # the factors of the edges the model kept
    for it in range(3):
        masks = [T(g["it%d.mask%d" % (it, k)]).to(d) for k in range(H + 2)]
        for h, att in enumerate(sg.attentions):
            att.draw_keep = (lambda mk: (lambda E, device: kept(mk).view(1, E)))(masks[h])
        sg.dropout_layer.forward = (lambda mk: (lambda x: x * mk))(masks[H])
        sg.out_att.draw_keep = (lambda mk: (lambda E, device: kept(mk).view(1, E)))(masks[H + 1])
        out_e, out_r, _ = m(None, T(g["it%d.batch_entities" % it]).to(d), (T(g["it%d.edge" % it]).to(d), T(g["it%d.edge_type" % it]).to(d)),
                            T(g["it%d.nhop" % it]).to(d))
        close(out_e, g["it%d.out_entity" % it], atol=2e-5, what="train-mode out_entity, iteration %d" % it)
        close(out_r, g["it%d.out_relation" % it], atol=2e-5, what="train-mode out_relation, iteration %d" % it)
        opt.zero_grad()
        loss = batch_gat_loss(loss_fn, T(g["it%d.train_indices" % it]).to(d), out_e, out_r, valid_invalid_ratio_gat=ratio)
        loss.backward()
        opt.step()
        np.testing.assert_allclose(loss.item(), g["losses"][it], rtol=1e-4, err_msg="loss of iteration %d" % it)
    for k, v in m.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), g["p3." + k], atol=1e-5, rtol=0, err_msg=k)
        if k not in ("entity_embeddings", "final_entity_embeddings", "final_relation_embeddings"):
            d_ref = g["p3." + k] - g["p0." + k]                                               # the three SGD updates themselves
            np.testing.assert_allclose(v.cpu().numpy() - g["p0." + k], d_ref, atol=5e-3 * np.abs(d_ref).max() + 1e-9, err_msg="delta " + k)


def test_optim_adam_convkb_training_step_matches_reference():
    """One ConvKB training step as the reference recorded it (GAT/main.py:747-751, :833-842), with recon_amd.optim.Adam doing the update:
    the reference's parameters after the step."""
    from recon_amd import kg_train
    from recon_amd.models import SpKBGATConvOnly
    from recon_amd.optim import Adam
    g = load_golden("convkb_train1")
    D = g["sd__final_entity_embeddings"].shape[1]
    m = SpKBGATConvOnly(torch.randn(int(g["n_ent"]), 8), torch.randn(int(g["n_rel"]), 8), [D // 2, D], [D // 2, D], 0.0, 0.0, 0.2, 0.2, [2, 2], 50)
    m.load_state_dict({k: T(g["sd__" + k]) for k in m.state_dict()}, strict=True)
    m = m.to(DEV)
    m.final_entity_embeddings.requires_grad_(False)
    m.final_relation_embeddings.requires_grad_(False)
    idx, val, ratio = T(g["step_indices"]).to(DEV), T(g["step_values"]).to(DEV), int(g["step_ratio"])
    opt = Adam(m.parameters(), lr=float(g["lr"]), weight_decay=float(g["weight_decay"]))
    opt.zero_grad()
    loss = kg_train.convkb_bce_loss(m, idx, val, ratio)
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * max(1.0, abs(float(g["loss"])))
    loss.backward()
    named = dict(m.named_parameters())
    trained = ("convKB.fc1.weight", "convKB.fc1.bias", "convKB.fc2.weight", "convKB.fc2.bias")
    for k in trained:
        ref = T(g["grad__" + k])
        torch.testing.assert_close(named[k].grad.cpu(), ref, rtol=1e-4, atol=1e-6 * float(ref.abs().max()) + 1e-9)
    untouched = {k: named[k].detach().clone() for k in ("convKB.conv_layer.weight", "convKB.fc_layer.weight", "final_entity_embeddings")}
    opt.step()
    for k in trained:
        torch.testing.assert_close(named[k].detach().cpu(), T(g["after__" + k]), rtol=1e-5, atol=1e-6)
    for k, v in untouched.items():
        assert named[k].grad is None and torch.equal(named[k].detach(), v)
