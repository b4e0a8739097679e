"""CPU-only: the parameter update's host statements (detector_step.step_host) against the reference's recorded steps
(tests/golden/detector_step.npz), the optimizer's state-dict format against torch.optim.SGD, the refusals, the table
bookkeeping and the C ABI surface of the two entries.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import detector_step_cases as cases
from conftest import ROOT

F32 = np.float32
U = 2.0 ** -24                  # float32's unit roundoff


@pytest.fixture(scope="module")
def ds():
    from event_representation_study_amd import detector_step
    return detector_step


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "detector_step.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def hosts(ds):
    """step_host over every golden case, once."""
    return {name: cases.run_host(cases.build(name)) for name in cases.GOLDEN}


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _skipped(c):
    return set(cases.GOLDEN[c["name"]].get("bad", {}))


def test_fixture_holds_the_cases_inputs(gold):
    """The gradients and hyper-parameters the maker fed are the ones the cases rebuild."""
    for name in cases.GOLDEN:
        c = cases.build(name)
        m = cases.model(c["seed"])
        pk = cases.param_keys(m)
        for t in range(c["steps"]):
            zeros = {k: np.zeros(tuple(p.shape), F32) for k, p in m.named_parameters()}
            g = cases.flat({k: c["grads"][t].get(k, zeros[k]) for k in pk}, pk)
            assert np.array_equal(_bits(gold[name + "/g"][t]), _bits(g)), (name, t)
            assert gold[name + "/has_grad"][t].tolist() == [k in c["grads"][t] for k in pk]
            lr, mom, _ = zip(*cases.groups_at(c, t))
            assert np.array_equal(gold[name + "/lr"][t], np.array(lr, np.float64)), (name, t)
            assert np.array_equal(gold[name + "/momentum"][t], np.array(mom, np.float64)), (name, t)
    for k in ("E_p", "E_buf", "E_ema"):
        assert 0 < float(gold["measured/" + k]) < 1e-6


@pytest.mark.parametrize("name", list(cases.GOLDEN))
def test_step_host_against_the_reference(gold, hosts, name):
    """Parameters, buffers and EMA entries within 4 x measured/E_* (the reference's own float32 rounding, relative to the
    greatest magnitude of the tensor in ref64) of ref32 at every recorded step; the EMA of entries no optimizer writes, the
    scale and the tracker bit for bit; a skipped step leaves parameters and buffers as they were."""
    c, h = cases.build(name), hosts[name]
    m = cases.model(c["seed"])
    pk, ek = cases.param_keys(m), cases.ema_keys(m)
    skipped = _skipped(c)
    for t in range(c["steps"]):
        has_buf = dict(zip(pk, gold[name + "/has_buf"][t]))
        for grp, keys in (("p", pk), ("buf", pk), ("ema", ek)):
            if name + "/" + grp not in gold:
                assert grp == "ema" and not c["ema"]
                continue
            E = float(gold["measured/E_" + grp])
            for k, (lo, hi) in cases.spans(m, keys).items():
                if grp == "buf" and not has_buf[k]:
                    assert np.isnan(h["buf"][t, lo:hi]).all(), (name, t, k)          # torch keeps none: ours was never written
                    continue
                got, ref, r64 = h[grp][t, lo:hi], gold[name + "/" + grp][t, lo:hi], gold[name + "/ref64_" + grp][t, lo:hi]
                err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()
                print("%s step %d %s %s: %.3g of %.3g" % (name, t, grp, k, err, 4 * E * np.abs(r64).max()))
                assert err <= 4 * E * np.abs(r64).max(), (name, t, grp, k)
                if grp == "ema" and k in cases.STATS:
                    assert np.array_equal(_bits(got), _bits(ref)), (name, t, k)       # an EMA-only update: bit for bit
        if c["scaler"]:
            assert np.array_equal(_bits(h["scale"][t]), _bits(gold[name + "/scale"][t])), (name, t)
            assert int(h["tracker"][t]) == int(gold[name + "/tracker"][t]), (name, t)
        if t in skipped:
            prev = h["p"][t - 1] if t else cases.flat({k: v.detach().numpy() for k, v in m.named_parameters()}, pk)
            assert np.array_equal(_bits(h["p"][t]), _bits(prev)), (name, t)
            if t:
                assert np.array_equal(_bits(h["buf"][t]), _bits(h["buf"][t - 1])), (name, t)
            else:
                assert np.isnan(h["buf"][t]).all()
        assert int(h["applied"][t]) == t + 1 - len([s for s in skipped if s <= t])
    assert skipped or name not in ("overflow_first", "overflow_mid")


def test_ema_statements_are_the_references_bits(gold, ds):
    """The two EMA statements on the reference's own float32 parameters reproduce its EMA entries bit for bit: what the issue
    states about torch's CPU route, held here for every parameter entry of every case."""
    for name in cases.GOLDEN:
        c = cases.build(name)
        if not c["ema"]:
            continue
        m = cases.model(c["seed"])
        pk, ek = cases.param_keys(m), cases.ema_keys(m)
        sp, se = cases.spans(m, pk), cases.spans(m, ek)
        e = cases.flat({k: v.numpy() for k, v in m.state_dict().items()}, ek).copy()
        for t in range(c["steps"]):
            hyper = ds.hyper_row((), ds.ema_decay(t + 1))
            for k in pk:
                rows = [dict(p=gold[name + "/p"][t, sp[k][0]:sp[k][1]], ema=e[se[k][0]:se[k][1]])]
                ds.step_host(rows, hyper, None, ema_only=True)
                assert np.array_equal(_bits(e[se[k][0]:se[k][1]]), _bits(gold[name + "/ema"][t, se[k][0]:se[k][1]])), (name, t, k)
            for k in cases.STATS:
                e[se[k][0]:se[k][1]] = gold[name + "/ema"][t, se[k][0]:se[k][1]]


def _bounds64(c, gold):
    """Per step the bound on |step_host - ref64| per tensor, see test_step_host_against_float64."""
    name = c["name"]
    m = cases.model(c["seed"])
    pk, ek = cases.param_keys(m), cases.ema_keys(m)
    sp, se = cases.spans(m, pk), cases.spans(m, ek)
    init = {k: float(v.abs().max()) for k, v in m.state_dict().items() if v.dtype.is_floating_point}
    ep, eb, ee = {k: 0.0 for k in pk}, {k: 0.0 for k in pk}, {k: 0.0 for k in ek}
    mx = lambda grp, t, span: float(np.abs(gold[name + "/ref64_" + grp][t, span[0]:span[1]]).max())
    out, applied = [], 0
    for t in range(c["steps"]):
        scale = 1.0 if not c["scaler"] else float(gold[name + "/scale"][t - 1] if t else c["scaler"][0])
        groups = cases.groups_at(c, t)
        skip = t in _skipped(c)
        for k in pk:
            if k in c["grads"][t] and not skip:
                lr, mom, wd = (float(v) for v in groups[cases.GROUP_OF[k]])
                G = float(np.abs(c["grads"][t][k]).max()) / scale
                P0 = mx("p", t - 1, sp[k]) if t else init[k]
                P1, B1 = mx("p", t, sp[k]), mx("buf", t, sp[k])
                B0 = mx("buf", t - 1, sp[k]) if applied else 0.0
                D = G + wd * P0
                D2 = D + mom * B1
                ed = U * (G + 2 * wd * P0 + D) + wd * ep[k]
                eb[k] = ed if applied == 0 else mom * eb[k] + 2 * U * mom * B0 + ed + U * B1
                ed2 = ed + mom * eb[k] + 2 * U * mom * B1 + U * D2
                ep[k] = ep[k] + lr * (ed2 + 2 * U * D2) + U * P1
        applied += 0 if skip else 1
        if c["ema"]:
            d = cases_decay(t + 1)
            for k in ek:
                E0 = mx("ema", t - 1, se[k]) if t else init[k]
                E1 = mx("ema", t, se[k])
                P1 = mx("p", t, sp[k]) if k in sp else float(np.abs(c["stats"][t][k]).max())
                ee[k] = d * ee[k] + 2 * U * d * E0 + (1 - d) * ep.get(k, 0.0) + 2 * U * (1 - d) * P1 + U * E1
        out.append((dict(ep), dict(eb), dict(ee)))
    return out


def cases_decay(updates):
    from event_representation_study_amd.detector_step import ema_decay
    return ema_decay(updates)


@pytest.mark.parametrize("name", list(cases.GOLDEN))
def test_step_host_against_float64(gold, hosts, name):
    """step_host against the reference's float64 run, within a bound that follows from the statements alone.

    u = 2^-24.  Every float32 operation adds at most u times the magnitude of its result; every hyper-parameter (lr, momentum,
    weight_decay, ema_d, ema_1md) is rounded to float32 once where the float64 run keeps the double, so a product with one
    carries 2u.  With G = max|g| / scale, P, B, E the greatest magnitudes of the tensor's parameter, buffer and EMA entry in
    ref64 (index 0 before the step, 1 after it), D = G + wd P0 >= |d| and D2 = D + mom B1 >= |d2|, the errors e. of one tensor obey
        e_d   <= u (G + 2 wd P0 + D) + wd e_p                       g * inv;  wd * p (2u) and e_p carried;  the sum
        e_buf <= e_d on the first applied step, else mom e_buf + 2u mom B0 + e_d + u B1
        e_d2  <= e_d + mom e_buf + 2u mom B1 + u D2
        e_p   <= e_p + lr (e_d2 + 2u D2) + u P1
        e_ema <= dcy e_ema + 2u dcy E0 + (1 - dcy) e_p + 2u (1 - dcy) P1 + u E1
    and a skipped step changes none of them.  Terms of order u^2 are covered by a factor 1.01.  The magnitudes come from the
    fixture, none from the code under test."""
    c, h = cases.build(name), hosts[name]
    m = cases.model(c["seed"])
    pk, ek = cases.param_keys(m), cases.ema_keys(m)
    sp, se = cases.spans(m, pk), cases.spans(m, ek)
    for t, (ep, eb, ee) in enumerate(_bounds64(c, gold)):
        has_buf = dict(zip(pk, gold[name + "/has_buf"][t]))
        for grp, spans, bound in (("p", sp, ep), ("buf", sp, eb), ("ema", se, ee)):
            if grp == "ema" and not c["ema"]:
                continue
            for k, (lo, hi) in spans.items():
                if grp == "buf" and not has_buf[k]:
                    continue
                err = np.abs(h[grp][t, lo:hi].astype(np.float64) - gold[name + "/ref64_" + grp][t, lo:hi]).max()
                print("%s step %d %s %s: %.3g of %.3g" % (name, t, grp, k, err, 1.01 * bound[k]))
                assert err <= 1.01 * bound[k], (name, t, grp, k)


def test_module_on_cpu_tensors_is_step_host(hosts):
    """SGD + GradScaler + ModelEMA + TrainStep on CPU tensors take step_host: bit for bit, every case and step."""
    for name in cases.GOLDEN:
        got, _ = cases.run_module(cases.build(name), "cpu")
        h = hosts[name]
        written = ~np.isnan(h["buf"])
        for k in ("p", "ema", "scale", "tracker", "applied"):
            assert np.array_equal(_bits(got[k]), _bits(h[k])) if got[k].dtype == F32 else np.array_equal(got[k], h[k]), (name, k)
        assert np.array_equal(_bits(got["buf"][written]), _bits(h["buf"][written])), name


def _steps(opt, params, grads):
    for g in grads:
        for p, v in zip(params, g):
            p.grad = v.clone()
        opt.step()


def _fresh(ds, kind, seed=5):
    m = cases.model(seed)
    if kind == "ours":
        return m, ds.build_optimizer(cases.cfg(), m)
    bn, w, b = [m.bn.weight], [m.conv1.weight, m.conv2.weight, m.fc.weight], [m.bn.bias, m.conv2.bias, m.fc.bias]
    opt = torch.optim.SGD(bn, lr=cases.LR0, momentum=cases.MOMENTUM, nesterov=True)
    opt.add_param_group({"params": w, "weight_decay": cases.WEIGHT_DECAY})
    opt.add_param_group({"params": b})
    return m, opt


@pytest.mark.parametrize("kind", ["ours", "torch"])
def test_state_dict_round_trips_with_torch_sgd(ds, kind):
    """ours -> torch.optim.SGD -> ours, and torch -> ours -> torch: the state dict loads on the other side, keeps torch's keys,
    and a step after the round trip is bit-equal to one without it."""
    other = "torch" if kind == "ours" else "ours"
    gen = torch.Generator().manual_seed(3)
    m, opt = _fresh(ds, kind)
    params = [p for g in opt.param_groups for p in g["params"]]
    grads = [[torch.randn(p.shape, generator=gen) for p in params] for _ in range(3)]
    _steps(opt, params, grads[:2])
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and sorted(sd["state"]) == list(range(7))
    assert all(set(st) == {"momentum_buffer"} and st["momentum_buffer"].dtype == torch.float32 for st in sd["state"].values())
    for a, b in zip(sd["param_groups"], _fresh(ds, "torch")[1].state_dict()["param_groups"]):
        assert set(a) == set(b) and a["params"] == b["params"]
    # through the other side and back
    m2, mid = _fresh(ds, other)
    mid.load_state_dict(sd)
    m3, back = _fresh(ds, kind)
    back.load_state_dict(mid.state_dict())
    with torch.no_grad():
        for q, p in zip(m3.parameters(), m.parameters()):
            q.copy_(p)
    params3 = [p for g in back.param_groups for p in g["params"]]
    _steps(opt, params, grads[2:])
    _steps(back, params3, grads[2:])
    for p, q in zip(params, params3):
        assert np.array_equal(_bits(p.detach().numpy()), _bits(q.detach().numpy()))
        assert np.array_equal(_bits(opt.state[p]["momentum_buffer"].numpy()), _bits(back.state[q]["momentum_buffer"].numpy()))


def _dyadic(m, opt):
    """Parameters in eighths and hyper-parameters that are powers of two: with whole-number gradients every operation of a
    few steps is exact in float32, so torch's route (which contracts its multiply-adds) and ours give the same bits."""
    with torch.no_grad():
        for p in m.parameters():
            p.copy_((p * 8).round() / 8)
    for group in opt.param_groups:                                      # (no weight decay: wd * p would add five bits a step)
        group["lr"], group["momentum"], group["weight_decay"] = 0.5, 0.5, 0.0


def test_buffers_replaced_between_two_train_steps_are_the_ones_stepped(ds):
    """load_state_dict, and an assignment to optimizer.state, between two TrainStep calls with an EMA attached: the step uses
    the new buffers, bit-equal to torch.optim.SGD from the same state, and optimizer.state holds what the step wrote."""
    gen = torch.Generator().manual_seed(11)
    m = cases.model(6)
    opt = ds.build_optimizer(cases.cfg(), m)
    _dyadic(m, opt)
    step = ds.TrainStep(opt, None, ds.ModelEMA(m))
    params = [p for g in opt.param_groups for p in g["params"]]
    whole = lambda p: torch.randint(-8, 9, p.shape, generator=gen).float()
    for p in params:
        p.grad = whole(p)
    for _ in range(2):
        step(m)
        for p in params:
            p.grad.copy_(whole(p))
    assert step.table_uploads == 1
    sd = opt.state_dict()
    for st in sd["state"].values():
        st["momentum_buffer"] = torch.full_like(st["momentum_buffer"], 100.0)
    # torch's optimizer on a copy of the model as it is now, from the same state
    m2, twin = _fresh(ds, "torch")
    with torch.no_grad():
        for q, p in zip(m2.parameters(), m.parameters()):
            q.copy_(p)
    twin.load_state_dict(sd)
    twin_params = [p for g in twin.param_groups for p in g["params"]]
    opt.load_state_dict(sd)
    held = [opt.state[p]["momentum_buffer"] for p in params]
    for p, q in zip(params, twin_params):
        q.grad = p.grad.clone()
    e0 = {k: v.detach().numpy().copy() for k, v in step.ema.ema.state_dict().items()}
    step(m)
    twin.step()
    assert step.table_uploads == 2
    for p, q, b in zip(params, twin_params, held):
        assert np.array_equal(_bits(p.detach().numpy()), _bits(q.detach().numpy()))
        assert opt.state[p]["momentum_buffer"] is b and not (b == 100.0).any()           # the loaded buffer is the one written
        assert np.array_equal(_bits(b.numpy()), _bits(twin.state[q]["momentum_buffer"].numpy()))
    hyper = ds.hyper_row((), ds.ema_decay(3))
    for k, p in m.named_parameters():                                   # and the EMA followed the parameters just written
        ds.step_host([dict(p=p.detach().numpy(), ema=e0[k])], hyper, None, ema_only=True)
        assert np.array_equal(_bits(step.ema.ema.state_dict()[k].numpy()), _bits(e0[k])), k
    # an assignment to optimizer.state is seen too
    p, q = params[1], twin_params[1]
    opt.state[p]["momentum_buffer"] = mine = torch.full_like(p, 3.0)
    twin.state[q]["momentum_buffer"] = torch.full_like(q, 3.0)
    for a, b in zip(params, twin_params):
        a.grad.copy_(whole(a))
        b.grad = a.grad.clone()
    step(m)
    twin.step()
    assert step.table_uploads == 3 and opt.state[p]["momentum_buffer"] is mine
    assert np.array_equal(_bits(mine.numpy()), _bits(twin.state[q]["momentum_buffer"].numpy()))
    assert all(np.array_equal(_bits(a.detach().numpy()), _bits(b.detach().numpy())) for a, b in zip(params, twin_params))


def test_ema_model_given_new_storage_is_noticed(ds):
    """.half() gives the EMA model's parameters new storage and another dtype: the next step refuses, naming the entry, and
    does not write through the old addresses; back in float32 the tables are made anew."""
    m = cases.model(7)
    opt = ds.build_optimizer(cases.cfg(), m)
    step = ds.TrainStep(opt, None, ds.ModelEMA(m))
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    step(m)
    step.ema.ema.half()
    with pytest.raises(ValueError, match=r"\(EMA\).*float16"):
        step(m)
    step.ema.ema.float()
    step(m)
    assert step.table_uploads == 2
    ema = ds.ModelEMA(m)
    ema.update(m)
    ema.ema.half()
    with pytest.raises(ValueError, match=r"\(EMA\).*float16"):
        ema.update(m)
    step.invalidate()                                                   # the public way to have everything listed anew
    step(m)
    assert step.table_uploads == 3


def test_refresh_makes_the_state_words(ds):
    """Nothing a launch needs is made by the launch: after refresh() the applied-steps word and the scaler's words exist."""
    m = cases.model(8)
    opt = ds.build_optimizer(cases.cfg(), m)
    scaler = ds.GradScaler(init_scale=8.0)
    scaler.update(new_scale=16.0)                                       # before any scale() or step(): taken as the first scale
    assert scaler.get_scale() == 16.0
    step = ds.TrainStep(opt, scaler, ds.ModelEMA(m))
    assert opt._applied is None and scaler._amp is None
    step.refresh(m)
    assert opt._applied is not None and scaler._amp is not None and scaler.get_scale() == 16.0
    scaler.update(new_scale=4.0)
    assert scaler.get_scale() == 4.0


def test_state_dict_before_any_applied_step_has_no_buffers(ds):
    m, opt = _fresh(ds, "ours")
    assert opt.state_dict()["state"] == {}
    scaler = ds.GradScaler(init_scale=4.0)
    for p in m.parameters():
        p.grad = torch.full_like(p, float("inf"))
    before = [p.detach().clone() for p in m.parameters()]
    scaler.step(opt)
    scaler.update()
    assert opt.applied_steps() == 0 and opt.state_dict()["state"] == {} and scaler.get_scale() == 2.0
    assert all(torch.equal(a, b) for a, b in zip(before, m.parameters()))
    torch.optim.SGD(list(m.parameters()), lr=0.1, momentum=0.9, nesterov=True)     # (and torch takes the empty state)
    _, t = _fresh(ds, "torch")
    t.load_state_dict(opt.state_dict())


def test_scaler_state_dict_speaks_torchs_keys(ds):
    ours = ds.GradScaler(init_scale=8.0, growth_interval=3, device="cpu")
    theirs = torch.amp.GradScaler("cpu", init_scale=8.0, growth_interval=3)
    theirs.scale(torch.zeros(()))
    assert set(ours.state_dict()) == set(theirs.state_dict())
    assert ours.state_dict() == theirs.state_dict()
    theirs.load_state_dict(ours.state_dict())
    sd = dict(theirs.state_dict(), scale=32.0, _growth_tracker=2)
    ours.load_state_dict(sd)
    assert ours.get_scale() == 32.0 and ours._get_growth_tracker() == 2
    off = ds.GradScaler(enabled=False)
    assert off.state_dict() == {} and off.get_scale() == 1.0 and off.scale(torch.ones(())).item() == 1.0
    with pytest.raises(RuntimeError):
        ours.update()                                                   # no step before it


def test_disabled_scaler_passes_through(ds):
    m, opt = _fresh(ds, "ours")
    m2, ref = _fresh(ds, "ours")
    for p, q in zip(m.parameters(), m2.parameters()):
        p.grad, q.grad = torch.ones_like(p), torch.ones_like(q)
    ds.GradScaler(enabled=False).step(opt)
    ref.step()
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), m2.parameters()))


def test_refusals_name_the_parameter(ds):
    m = cases.model(1)
    m.conv2.weight = torch.nn.Parameter(m.conv2.weight.detach().double())
    with pytest.raises(ValueError, match=r"conv2\.weight.*float64"):
        ds.build_optimizer(cases.cfg(), m)
    m = cases.model(1)
    m.conv1.weight = torch.nn.Parameter(torch.randn(3, 5, 3, 3).permute(1, 0, 2, 3))
    assert not m.conv1.weight.is_contiguous()
    with pytest.raises(ValueError, match=r"conv1\.weight.*not contiguous"):
        ds.build_optimizer(cases.cfg(), m)
    m = cases.model(1)
    m.fc.bias = torch.nn.Parameter(torch.empty(3, device="meta"))
    with pytest.raises(ValueError, match=r"fc\.bias.*meta.*share a device"):
        ds.build_optimizer(cases.cfg(), m)
    # the EMA's entries are held to the same rules, by their key
    m = cases.model(1)
    opt, ema = ds.build_optimizer(cases.cfg(), m), ds.ModelEMA(m)
    ema.ema.bn.running_mean = ema.ema.bn.running_mean.double()
    with pytest.raises(ValueError, match=r"bn\.running_mean.*float64"):
        ds.TrainStep(opt, None, ema)(m)
    with pytest.raises(ValueError, match=r"bn\.running_mean.*float64"):
        ema.update(m)


def test_what_is_not_mirrored_says_so(ds):
    m = cases.model(1)
    cfg = cases.cfg()
    cfg.solver.optim = "Adam"
    with pytest.raises(NotImplementedError):
        ds.build_optimizer(cfg, m)
    ps = list(m.parameters())
    with pytest.raises(NotImplementedError):
        ds.SGD(ps, lr=0.1, momentum=0.9, nesterov=False)
    with pytest.raises(NotImplementedError):
        ds.SGD(ps, lr=0.1, momentum=0.9, nesterov=True, dampening=0.1)
    with pytest.raises(NotImplementedError):
        ds.SGD(ps, lr=0.1, maximize=True)
    opt = ds.SGD(ps, lr=0.1, momentum=0.9, nesterov=True)
    opt.param_groups[0]["nesterov"] = False                             # written later: held at the next table build
    opt._table.invalidate()
    with pytest.raises(NotImplementedError):
        opt.step()
    with pytest.raises(TypeError):
        ds.TrainStep(torch.optim.SGD(ps, lr=0.1))
    with pytest.raises(TypeError):
        ds.GradScaler(device="cpu").step(torch.optim.SGD(ps, lr=0.1))


def test_empty_tensor_is_allowed_and_plain_sgd_momentum_zero(ds):
    empty, p = torch.nn.Parameter(torch.empty(0)), torch.nn.Parameter(torch.tensor([1.0, -2.0]))
    opt = ds.SGD([empty, p], lr=0.5)                                    # momentum 0: d2 = d, the buffer is not touched
    empty.grad, p.grad = torch.empty(0), torch.tensor([2.0, 2.0])
    opt.step()
    assert p.detach().tolist() == [0.0, -3.0] and p.grad.tolist() == [0.0, 0.0]
    assert opt.state_dict()["state"] == {} and "momentum_buffer" not in opt.state.get(p, {})    # plain SGD keeps no buffer


def test_group_order_and_arguments_are_the_references(ds):
    m = cases.model(2)
    opt = ds.build_optimizer(cases.cfg(), m)
    names = {id(p): k for k, p in m.named_parameters()}
    assert [[names[id(p)] for p in g["params"]] for g in opt.param_groups] == \
        [[k for k in names.values() if cases.GROUP_OF[k] == i] for i in range(3)] == \
        [["bn.weight"], ["conv1.weight", "conv2.weight", "fc.weight"], ["bn.bias", "conv2.bias", "fc.bias"]]
    assert [g["weight_decay"] for g in opt.param_groups] == [0, cases.WEIGHT_DECAY, 0]
    assert all(g["lr"] == cases.LR0 and g["momentum"] == cases.MOMENTUM and g["nesterov"] for g in opt.param_groups)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda e: 0.5 ** e)
    assert all(g["initial_lr"] == cases.LR0 for g in opt.param_groups)
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    opt.step()
    sched.step()
    assert all(g["lr"] == cases.LR0 * 0.5 for g in opt.param_groups)


def test_tables_are_uploaded_once_while_the_gradients_stay(ds):
    m = cases.model(3)
    opt = ds.build_optimizer(cases.cfg(), m)
    step = ds.TrainStep(opt, ds.GradScaler(init_scale=2.0), ds.ModelEMA(m))
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    for _ in range(10):
        step(m)
        for p in m.parameters():
            p.grad.add_(1.0)                                            # what backward does to a gradient that is there
    assert step.table_uploads == 1 and opt.applied_steps() == 10
    m.fc.weight.grad = torch.ones_like(m.fc.weight)                     # replaced: another address
    step(m)
    assert step.table_uploads == 2
    m.fc.bias.grad = None                                               # and None is a change too
    before = m.fc.bias.detach().clone()
    step(m)
    assert step.table_uploads == 3 and torch.equal(before, m.fc.bias)
    step(m)
    assert step.table_uploads == 3
    # the optimizer on its own keeps its own table
    for _ in range(3):
        opt.step()
    assert opt.table_uploads == 1
    # a frozen parameter is not stepped and still averaged
    m.conv1.weight.requires_grad_(False)
    m.conv1.weight.grad = torch.ones_like(m.conv1.weight)
    before, e0 = m.conv1.weight.detach().clone(), step.ema.ema.conv1.weight.detach().clone()
    step(m)
    assert torch.equal(before, m.conv1.weight) and not torch.equal(e0, step.ema.ema.conv1.weight)


def test_model_ema_keeps_the_references_surface(ds):
    m = cases.model(4)
    ema = ds.ModelEMA(m, decay=0.99, updates=7)
    assert ema.updates == 7 and not ema.ema.training and not any(p.requires_grad for p in ema.ema.parameters())
    assert ema.decay(10) == 0.99 * (1 - np.exp(-10 / 2000))
    m.stride, m._private = 32, 1
    ema.update_attr(m, include=("stride",))
    assert ema.ema.stride == 32 and not hasattr(ema.ema, "_private")
    with torch.no_grad():
        m.bn.num_batches_tracked += 5
        for p in m.parameters():
            p.add_(1.0)
    e0 = {k: v.clone() for k, v in ema.ema.state_dict().items()}
    ema.update(m)
    d = ema.decay(8)
    assert ema.updates == 8 and int(ema.ema.bn.num_batches_tracked) == 0
    for k, v in ema.ema.state_dict().items():
        if v.dtype.is_floating_point:
            want = e0[k].numpy() * F32(d)
            want = want + F32(1 - d) * m.state_dict()[k].numpy()
            assert np.array_equal(_bits(v.numpy()), _bits(want)), k


def _header():
    return open(os.path.join(ROOT, "include", "evrep.h")).read()


def test_entries_are_declared_and_bound(ds):
    """The C ABI surface of the two entries, in the manner of test_capi_cpu.py: the symbols, their argument counts, the two
    structs and every constant of the header against _lib.py and the numpy records the tables are built with."""
    from event_representation_study_amd import build, _lib
    build.build()
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, nargs in (("evrep_train_step", 13), ("evrep_ema_update", 6)):
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(decl.split(",")) == nargs == len(_lib.SYMBOLS[name][1])
        assert isinstance(_lib.SYMBOLS[name], _lib.Status) and getattr(lib, name) is not None
    assert ctypes.sizeof(_lib.StepTensor) == 48 == ds.TENSOR_DTYPE.itemsize and ctypes.sizeof(_lib.StepChunk) == 16 == ds.CHUNK_DTYPE.itemsize
    for struct, dtype in ((_lib.StepTensor, ds.TENSOR_DTYPE), (_lib.StepChunk, ds.CHUNK_DTYPE)):
        assert [(n, getattr(struct, n).offset) for n, _ in struct._fields_] == [(n, dtype.fields[n][1]) for n in dtype.names]
    defines = {n: int(v) for n, v in re.findall(r"^#define\s+EVREP_(STEP_[A-Z_]+)\s+(\d+)u?\b", _header(), flags=re.M)}
    assert defines == {n: v for n, v in vars(_lib).items() if n.startswith("STEP_")} and len(defines) == 10
    assert _lib.STEP_CHUNK % 1024 == 0


def test_c_entries_refuse_before_any_launch():
    """Every refusal is EVREP_EINVAL before a launch, so made-up addresses are safe here with or without a device."""
    from event_representation_study_amd import build, _lib
    build.build()
    lib = _lib.load()
    vp = ctypes.c_void_p
    T, C, H, A, S = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000

    def step(t=T, nt=2, c=C, nc=3, h=H, ng=3, amp=A, applied=S, growth=2.0, backoff=0.5, interval=2000, flags=1):
        return lib.evrep_train_step(vp(t), nt, vp(c), nc, vp(h), ng, vp(amp), vp(applied), growth, backoff, interval, flags, None)

    refused = dict(no_tensors=dict(t=None), tensors_misaligned=dict(t=T + 4), no_chunks=dict(c=None), chunks_misaligned=dict(c=C + 4),
                   no_hyper=dict(h=None), hyper_misaligned=dict(h=H + 2), amp_misaligned=dict(amp=A + 2), no_applied=dict(applied=None),
                   applied_misaligned=dict(applied=S + 2), negative_tensors=dict(nt=-1), negative_chunks=dict(nc=-1),
                   too_many_chunks=dict(nc=1 << 31), chunks_without_tensors=dict(nt=0, t=None), no_groups=dict(ng=0),
                   too_many_groups=dict(ng=_lib.STEP_MAX_GROUPS + 1), unknown_flag=dict(flags=8), growth_nan=dict(growth=float("nan")),
                   growth_inf=dict(growth=float("inf")), backoff_zero=dict(backoff=0.0), interval_zero=dict(interval=0))
    for what, kw in refused.items():
        assert step(**kw) == _lib.EVREP_EINVAL, what

    def ema(t=T, nt=2, c=C, nc=3, h=H):
        return lib.evrep_ema_update(vp(t), nt, vp(c), nc, vp(h), None)

    for what, kw in dict(no_tensors=dict(t=None), no_chunks=dict(c=None), no_hyper=dict(h=None), misaligned=dict(c=C + 2),
                         negative=dict(nc=-1), chunks_without_tensors=dict(nt=0, t=None)).items():
        assert ema(**kw) == _lib.EVREP_EINVAL, what
    assert ema(nc=0, c=None, nt=0, t=None) == _lib.EVREP_OK             # nothing to do: no launch
