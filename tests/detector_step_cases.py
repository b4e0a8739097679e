"""The cases of the parameter update (event_representation_study_amd/detector_step.py), shared by the golden maker
(tests/golden/make_golden_detector_step.py) and the tests: a tiny model of our own whose parameters fall into all three groups
of the reference's ``build_optimizer``, and per case a seeded sequence of steps -- the gradients fed, the ``lr`` / ``momentum``
written into each group, the BN running statistics a forward pass would have left.

    name            steps  scaler (init, interval)   EMA   stands on
    shipped           4    1024, 2000                yes   lr0 0.0032, momentum 0.843, weight_decay 0.00036
    warmup            5    1024, 2000                yes   lr and momentum rewritten per group on every step, the bias group apart
    overflow_first    4    1024, 2000                yes   an inf in the first step's gradients: skipped, backoff, buffers stay absent
    overflow_mid      5    1024, 2000                yes   a NaN in the third step's gradients
    growth            5    1024, 2                   yes   the scale doubles after every second clean step
    no_wd             3    1024, 2000                yes   weight_decay = 0 in every group
    no_grad_param     3    1024, 2000                yes   fc.bias never receives a gradient: not stepped, still averaged
    no_scaler         3    none                      yes   the gradients are taken as they are
    no_ema            3    1024, 2000                no    the step alone

The groups, in the reference's order: 0 the BatchNorm2d weights (bn.weight), 1 the other weights with weight decay
(conv1.weight, conv2.weight, fc.weight), 2 the biases (bn.bias, conv2.bias, fc.bias).
"""
import types

import numpy as np
import torch

F32 = np.float32
LR0, MOMENTUM, WEIGHT_DECAY = 0.0032, 0.843, 0.00036
WARMUP_BIAS_LR, WARMUP_MOMENTUM, WARMUP_STEPS = 0.1, 0.5, 4

#        name: dict(seed, steps, scaler (init_scale, growth_interval) or None, ema, ...)
GOLDEN = {
    "shipped": dict(seed=31, steps=4, scaler=(1024.0, 2000), ema=True),
    "warmup": dict(seed=32, steps=5, scaler=(1024.0, 2000), ema=True, warmup=True),
    "overflow_first": dict(seed=33, steps=4, scaler=(1024.0, 2000), ema=True, bad={0: np.inf}),
    "overflow_mid": dict(seed=34, steps=5, scaler=(1024.0, 2000), ema=True, bad={2: np.nan}),
    "growth": dict(seed=35, steps=5, scaler=(1024.0, 2), ema=True),
    "no_wd": dict(seed=36, steps=3, scaler=(1024.0, 2000), ema=True, weight_decay=0.0),
    "no_grad_param": dict(seed=37, steps=3, scaler=(1024.0, 2000), ema=True, no_grad=("fc.bias",)),
    "no_scaler": dict(seed=38, steps=3, scaler=None, ema=True),
    "no_ema": dict(seed=39, steps=3, scaler=(1024.0, 2000), ema=False),
}


class Tiny(torch.nn.Module):
    """Conv + BN + biased Conv + Linear: every group of ``build_optimizer`` is populated, and BN brings float buffers and an
    integer one into the state dict."""

    def __init__(self):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(3, 5, 3, bias=False)
        self.bn = torch.nn.BatchNorm2d(5)
        self.conv2 = torch.nn.Conv2d(5, 4, 1, bias=True)
        self.fc = torch.nn.Linear(4, 3)


def model(seed, dtype=torch.float32):
    """The case's model: every parameter and float buffer drawn from the case's generator, not from torch's."""
    rng = np.random.default_rng(seed)
    m = Tiny()
    with torch.no_grad():
        for _, t in sorted(m.state_dict().items()):
            if t.dtype.is_floating_point:
                t.copy_(torch.from_numpy(rng.normal(size=tuple(t.shape)).astype(F32)))
        m.bn.running_var.abs_().add_(0.5)
    return m.to(dtype)


def cfg(weight_decay=WEIGHT_DECAY):
    """What ``build_optimizer`` reads of a config."""
    return types.SimpleNamespace(solver=types.SimpleNamespace(optim="SGD", lr0=LR0, momentum=MOMENTUM, weight_decay=weight_decay))


def param_keys(m):
    return [k for k, _ in m.named_parameters()]


def ema_keys(m):
    return [k for k, t in m.state_dict().items() if t.dtype.is_floating_point]


def build(name):
    """The case as a dict: seed, steps, scaler, ema, weight_decay, no_grad, and per step t
    grads[t]   {parameter key: float32 array}, as stored in ``.grad`` (that is: scaled); a key of no_grad is missing
    lr[t], momentum[t]   three values each (np.float64, as ``np.interp`` leaves them in the reference's warm-up), or None where
                         the groups keep what ``build_optimizer`` gave them
    stats[t]   {"bn.running_mean", "bn.running_var": float32 array}: what a forward pass left in the model's buffers."""
    spec = GOLDEN[name]
    rng = np.random.default_rng(spec["seed"] + 1000)
    m = model(spec["seed"])
    shapes = {k: tuple(p.shape) for k, p in m.named_parameters()}
    no_grad = tuple(spec.get("no_grad", ()))
    mag = F32(spec["scaler"][0] if spec["scaler"] else 1.0)
    c = dict(name=name, seed=spec["seed"], steps=spec["steps"], scaler=spec["scaler"], ema=spec["ema"],
             weight_decay=spec.get("weight_decay", WEIGHT_DECAY), no_grad=no_grad, grads=[], lr=[], momentum=[], stats=[])
    keys = [k for k in shapes if k not in no_grad]
    for t in range(spec["steps"]):
        g = {k: (rng.normal(size=shapes[k]).astype(F32) * mag) for k in keys}
        if t in spec.get("bad", {}):
            last = g[keys[-1]].reshape(-1)
            last[-1] = spec["bad"][t]
        c["grads"].append(g)
        if spec.get("warmup"):
            lr = [np.interp(t + 1, [0, WARMUP_STEPS], [WARMUP_BIAS_LR if k == 2 else 0.0, LR0]) for k in range(3)]
            mom = [np.interp(t + 1, [0, WARMUP_STEPS], [WARMUP_MOMENTUM, MOMENTUM])] * 3
            c["lr"].append(lr)
            c["momentum"].append(mom)
        else:
            c["lr"].append(None)
            c["momentum"].append(None)
        c["stats"].append({"bn.running_mean": rng.normal(size=5).astype(F32), "bn.running_var": (rng.random(5) + 0.5).astype(F32)})
    return c


GROUP_OF = {"bn.weight": 0, "conv1.weight": 1, "conv2.weight": 1, "fc.weight": 1, "bn.bias": 2, "conv2.bias": 2, "fc.bias": 2}
STATS = ("bn.running_mean", "bn.running_var")


def groups_at(c, t):
    """The three groups' (lr, momentum, weight_decay) at step t, as Python / numpy doubles."""
    lr, mom = c["lr"][t] or [LR0] * 3, c["momentum"][t] or [MOMENTUM] * 3
    return [(lr[k], mom[k], c["weight_decay"] if k == 1 else 0.0) for k in range(3)]


def run_host(c, amp_consts=(2.0, 0.5)):
    """The case through ``detector_step.step_host`` alone, on numpy arrays: the recorded arrays of the fixture's layout
    (p, buf, ema, scale, tracker, applied per step) and the zeroed gradients."""
    from event_representation_study_amd import detector_step as ds
    m = model(c["seed"])
    pk, ek = param_keys(m), ema_keys(m)
    sd = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    ema = {k: sd[k].copy() for k in ek} if c["ema"] else {}
    buf = {k: np.full_like(sd[k], np.nan) for k in pk}                   # never read before the first applied step
    state = ds.new_state(scale=c["scaler"][0] if c["scaler"] else 1.0)
    amp = (amp_consts[0], amp_consts[1], c["scaler"][1]) if c["scaler"] else None
    out = {k: [] for k in ("p", "buf", "ema", "scale", "tracker", "applied")}
    for t in range(c["steps"]):
        for k in STATS:
            sd[k][...] = c["stats"][t][k]
        g = {k: v.copy() for k, v in c["grads"][t].items()}
        rows = [dict(p=sd[k], g=g.get(k), buf=buf[k] if k in g else None, ema=ema.get(k), group=GROUP_OF[k],
                     flags=(ds.HAS_GRAD if k in g else 0) | (ds.HAS_EMA if c["ema"] else 0)) for k in pk]
        rows += [dict(p=sd[k], g=None, buf=None, ema=ema[k], group=0, flags=ds.HAS_EMA | ds.EMA_ONLY) for k in ek if k not in pk and c["ema"]]
        hyper = ds.hyper_row(groups_at(c, t), ds.ema_decay(t + 1) if c["ema"] else None)
        ds.step_host(rows, hyper, state, amp)
        assert all((v == 0).all() and not np.signbit(v).any() for v in g.values())
        out["p"].append(flat(sd, pk))
        out["buf"].append(flat(buf, pk))
        out["ema"].append(flat(ema, ek) if c["ema"] else np.zeros(0, F32))
        out["scale"].append(F32(state["scale"]))
        out["tracker"].append(np.int32(state["tracker"]))
        out["applied"].append(np.int32(state["applied_steps"]))
    return {k: np.stack(v) for k, v in out.items()}


def rehome(module, arena):
    """Move every parameter and buffer of `module` into guarded regions of `arena` (tests/guarded.py), values kept."""
    for t in list(module.parameters()) + list(module.buffers()):
        t.data = arena.carve_like(t.data, readonly=False)
    return module


def run_module(c, device="cpu", zero_grad=True, arena=None):
    """The case end to end through ``build_optimizer`` + ``GradScaler`` + ``ModelEMA`` + ``TrainStep`` on `device`: the same
    arrays as ``run_host``, and the objects.  With `arena` every tensor the step touches -- model, EMA model, gradients, momentum
    buffers -- is carved from it, and its guard bands are checked after every step."""
    from event_representation_study_amd import detector_step as ds
    m = model(c["seed"]).to(device)
    if arena is not None:
        rehome(m, arena)
    pk, ek = param_keys(m), ema_keys(m)
    params, buffers = dict(m.named_parameters()), dict(m.named_buffers())
    opt = ds.build_optimizer(cfg(c["weight_decay"]), m, zero_grad=zero_grad)
    ema = ds.ModelEMA(m) if c["ema"] else None
    scaler = ds.GradScaler(init_scale=c["scaler"][0], growth_interval=c["scaler"][1]) if c["scaler"] else None
    step = ds.TrainStep(opt, scaler, ema)
    grads = {k: torch.zeros_like(p) for k, p in params.items() if k not in c["no_grad"]}
    if arena is not None:
        if ema:
            rehome(ema.ema, arena)
        grads = {k: arena.carve_like(g, readonly=False) for k, g in grads.items()}
        for k in grads:                                                  # -0.0: what the optimizer itself starts a buffer with
            opt.state[params[k]]["momentum_buffer"] = arena.carve_like(torch.full_like(params[k].data, -0.0), readonly=False)
    out = {k: [] for k in ("p", "buf", "ema", "scale", "tracker", "applied")}
    host = lambda t: t.detach().cpu().numpy()
    for t in range(c["steps"]):
        if c["lr"][t] is not None:
            for k, group in enumerate(opt.param_groups):
                group["lr"], group["momentum"] = c["lr"][t][k], c["momentum"][t][k]
        with torch.no_grad():
            for k in STATS:
                buffers[k].copy_(torch.from_numpy(c["stats"][t][k]))
            m.bn.num_batches_tracked += 1
            for k, g in grads.items():                                   # the gradient tensors stay where they are, as after backward
                g.copy_(torch.from_numpy(c["grads"][t][k]))
                params[k].grad = g
        step(m)
        if arena is not None:
            arena.check()
        if zero_grad:
            assert all((host(g) == 0).all() and not np.signbit(host(g)).any() for g in grads.values())
        nan = {k: np.full(tuple(p.shape), np.nan, F32) for k, p in params.items()}
        out["p"].append(flat({k: host(p) for k, p in params.items()}, pk))
        out["buf"].append(flat({k: host(opt.state[p]["momentum_buffer"]) if "momentum_buffer" in opt.state.get(p, {}) else nan[k]
                                for k, p in params.items()}, pk))
        out["ema"].append(flat({k: host(v) for k, v in ema.ema.state_dict().items()}, ek) if ema else np.zeros(0, F32))
        out["scale"].append(F32(scaler.get_scale() if scaler else 1.0))
        out["tracker"].append(np.int32(scaler._get_growth_tracker() if scaler else 0))
        out["applied"].append(np.int32(opt.applied_steps()))
    return {k: np.stack(v) for k, v in out.items()}, dict(model=m, optimizer=opt, ema=ema, scaler=scaler, step=step)


def flat(tensors, keys):
    """{key: array-like} -> one vector in the order of `keys`."""
    return np.concatenate([np.asarray(tensors[k]).reshape(-1) for k in keys]) if keys else np.zeros(0, F32)


def spans(m, keys):
    """{key: (start, stop)} of `flat`'s vector."""
    sd, out, off = dict(m.state_dict()), {}, 0
    for k in keys:
        n = sd[k].numel()
        out[k] = (off, off + n)
        off += n
    return out
