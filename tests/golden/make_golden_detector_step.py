#!/usr/bin/env python3
"""Golden vectors for the parameter update (tests/golden/detector_step.npz).

Run where the reference lies (the fixture travels, the reference does not), naming its root:

    python tests/golden/make_golden_detector_step.py <root of the reference checkout>

The reference's own ``build_optimizer`` (``ev-YOLOv6/yolov6/solver/build.py``) and ``ModelEMA`` (``yolov6/utils/ema.py``) are
IMPORTED from where they lie, never copied, and run on CPU tensors with torch's own ``torch.amp.GradScaler("cpu", ...)`` in the
order of ``yolov6/core/engine.py:547-552``: ``scaler.step(optimizer)``, ``scaler.update()``, ``optimizer.zero_grad()``,
``ema.update(model)``.  What this image lacks is an empty in-process stand-in, as in make_golden_detector_assign.py.

The cases are tests/detector_step_cases.py's GOLDEN, on its tiny model.  Per step the maker writes the case's ``lr`` / ``momentum``
into the groups (where the case has them), the case's running statistics into the model's BN buffers, and the case's gradients
into ``.grad``.  Recorded per case, first axis the step:
  g, has_grad           the gradients fed, flattened in named_parameters() order (0 where a parameter has none), and which have one
  lr, momentum          the three groups' values as set
  p, buf, has_buf       parameters and momentum buffers after the step (0 where torch keeps none), and which buffers exist
  ema                   the EMA model's floating entries after the step, flattened in state-dict order (without EMA: absent)
  scale, tracker        the scaler's float32 scale and int32 growth tracker after the step (without a scaler: absent)
and the same from a run with the model, its gradients and the EMA model in float64 under ``ref64_p``, ``ref64_buf``, ``ref64_ema``.
MEASURED and stored under ``measured/E_p``, ``E_buf``, ``E_ema``: the greatest |ref32 - ref64| of a tensor relative to the greatest
magnitude of that tensor in ref64, over all cases, steps and tensors.  The reference's own float32 rounding.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import detector_step_cases as cases  # noqa: E402
from make_golden_detector_assign import _reference as _reference_assign  # noqa: E402  (the stand-ins and the import path)

OUT = os.path.join(HERE, "detector_step.npz")


def _reference(root):
    _reference_assign(root)
    from yolov6.solver.build import build_optimizer
    from yolov6.utils.ema import ModelEMA
    return build_optimizer, ModelEMA


def run_reference(build_optimizer, ModelEMA, c, dtype):
    m = cases.model(c["seed"], dtype)
    pk, ek = cases.param_keys(m), cases.ema_keys(m)
    params = dict(m.named_parameters())
    opt = build_optimizer(cases.cfg(c["weight_decay"]), m)
    assert [len(g["params"]) for g in opt.param_groups] == [1, 3, 3]
    ema = ModelEMA(m) if c["ema"] else None
    scaler = torch.amp.GradScaler("cpu", init_scale=c["scaler"][0], growth_interval=c["scaler"][1]) if c["scaler"] else \
        torch.amp.GradScaler("cpu", enabled=False)
    out = {k: [] for k in ("g", "has_grad", "lr", "momentum", "p", "buf", "has_buf", "ema", "scale", "tracker")}
    for t in range(c["steps"]):
        if c["lr"][t] is not None:
            for k, group in enumerate(opt.param_groups):
                group["lr"], group["momentum"] = c["lr"][t][k], c["momentum"][t][k]
        with torch.no_grad():
            for key, v in c["stats"][t].items():
                dict(m.named_buffers())[key].copy_(torch.from_numpy(v))
            m.bn.num_batches_tracked += 1
        for key, p in params.items():
            p.grad = torch.from_numpy(c["grads"][t][key].copy()).to(dtype) if key in c["grads"][t] else None
        scaler.scale(torch.zeros(()))                                    # the scale comes to life in scale(), as in a real step
        scaler.step(opt)
        scaler.update()
        opt.zero_grad()
        if ema:
            ema.update(m)
        zeros = {k: np.zeros(tuple(p.shape)) for k, p in params.items()}
        bufs = {k: opt.state.get(p, {}).get("momentum_buffer") for k, p in params.items()}
        out["g"].append(cases.flat({k: c["grads"][t].get(k, zeros[k]) for k in pk}, pk))
        out["has_grad"].append(np.array([k in c["grads"][t] for k in pk]))
        out["lr"].append(np.array([float(g["lr"]) for g in opt.param_groups]))
        out["momentum"].append(np.array([float(g["momentum"]) for g in opt.param_groups]))
        out["p"].append(cases.flat({k: p.detach().numpy() for k, p in params.items()}, pk))
        out["buf"].append(cases.flat({k: (zeros[k] if b is None else b.numpy()) for k, b in bufs.items()}, pk))
        out["has_buf"].append(np.array([bufs[k] is not None for k in pk]))
        if ema:
            out["ema"].append(cases.flat({k: v.numpy() for k, v in ema.ema.state_dict().items()}, ek))
            assert int(ema.ema.bn.num_batches_tracked) == 0             # integer entries are left alone
        if c["scaler"]:
            assert scaler._scale.dtype == torch.float32 and scaler._growth_tracker.dtype == torch.int32
            out["scale"].append(scaler._scale.numpy().copy())
            out["tracker"].append(scaler._growth_tracker.numpy().copy())
    return {k: np.stack(v) for k, v in out.items() if v}, m


def main(root):
    build_optimizer, ModelEMA = _reference(root)
    out, worst = {}, dict(E_p=0.0, E_buf=0.0, E_ema=0.0)
    for name in cases.GOLDEN:
        c = cases.build(name)
        r32, m = run_reference(build_optimizer, ModelEMA, c, torch.float32)
        r64, _ = run_reference(build_optimizer, ModelEMA, c, torch.float64)
        assert r32["p"].dtype == np.float32 and r64["p"].dtype == np.float64
        for k in ("has_grad", "has_buf", "scale", "tracker"):
            assert k not in r32 or np.array_equal(r32[k], r64[k]), (name, k)
        e = {}
        for grp, keys in (("p", cases.param_keys(m)), ("buf", cases.param_keys(m)), ("ema", cases.ema_keys(m))):
            if grp not in r32:
                continue
            e["E_" + grp] = 0.0
            for k, (lo, hi) in cases.spans(m, keys).items():
                for t in range(c["steps"]):
                    a, b = r32[grp][t, lo:hi].astype(np.float64), r64[grp][t, lo:hi]
                    assert np.isfinite(a).all() and np.isfinite(b).all(), (name, grp, k)
                    if np.abs(b).max() > 0:
                        e["E_" + grp] = max(e["E_" + grp], float(np.abs(a - b).max() / np.abs(b).max()))
        for k, v in e.items():
            worst[k] = max(worst[k], v)
        for k, v in r32.items():
            out[name + "/" + k] = v
        for k in ("p", "buf", "ema"):
            if k in r64:
                out[name + "/ref64_" + k] = r64[k]
        print("%-15s " % name + " ".join("%s %.3g" % kv for kv in e.items())
              + ("  scale %s tracker %s" % (r32["scale"].tolist(), r32["tracker"].tolist()) if "scale" in r32 else ""))
    for k, v in worst.items():
        out["measured/" + k] = np.float64(v)
        print("measured/%-6s %.6g" % (k, v))
    np.savez_compressed(OUT, **out)
    print("->", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
