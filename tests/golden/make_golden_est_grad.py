#!/usr/bin/env python3
"""Golden gradients for the EST quantisation layer: the reference's own QuantizationLayer (ev-YOLOv6/yolov6/models/
learned_repr.py) run forward and backward on the CPU, with the stand-ins of make_golden_est.py.

    python tests/golden/make_golden_est_grad.py <checkout of uzh-rpg/event_representation_study>

The value MLP and the events are those of est.npz (C, H, W = 6, 48, 64; three items of 4000 / 1500 / 2500 events).  The loss is
(Wt * forward(events)).sum() with Wt = default_rng(seed).standard_normal(shape, float32) -- float32 so that both runs see the
same numbers; the seed is stored, not the array.  Two runs per image_size (96 and None): as the reference runs (float32), and
with the value layer and the events cast to float64.  Stored: the six weight gradients of every run, the weights, the events.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20240


def loss_weights(shape, seed=SEED):
    return np.random.default_rng(seed).standard_normal(tuple(shape), dtype=np.float32)


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        raise SystemExit(__doc__)
    spec = importlib.util.spec_from_file_location(
        "ref_learned_repr", os.path.join(sys.argv[1], "ev-YOLOv6", "yolov6", "models", "learned_repr.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    torch.set_num_threads(1)
    src = np.load(os.path.join(HERE, "est.npz"))
    C, H, W = (int(v) for v in src["dim"])
    ev = src["events"]
    state = {k[2:]: torch.from_numpy(src[k]) for k in src.files if k.startswith("w_")}
    torch.Tensor.cuda = lambda self, *a, **k: self
    g = {"dim": np.array([C, H, W]), "seed": SEED, "events": ev, "image_sizes": np.array([96, 0])}   # 0: image_size None
    for k, v in state.items():
        g["w_" + k] = v.numpy()
    for size in (96, None):
        for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            vl = m.ValueLayer.__new__(m.ValueLayer)            # without the constructor's own initialisation (:24-30)
            torch.nn.Module.__init__(vl)
            vl.activation = torch.nn.LeakyReLU(negative_slope=0.1)
            vl.mlp = torch.nn.ModuleList([torch.nn.Linear(1, 100), torch.nn.Linear(100, 100), torch.nn.Linear(100, 1)])
            vl.load_state_dict(state)
            vl = vl.to(dtype)
            q = m.QuantizationLayer.__new__(m.QuantizationLayer)
            torch.nn.Module.__init__(q)
            q.value_layer, q.dim, q.image_size = vl, (C, H, W), size
            if size is None:
                q.crop_and_resize_to_resolution = lambda x: x
            out = q.forward(torch.from_numpy(ev.copy()).to(dtype))
            wt = torch.from_numpy(loss_weights(out.shape))
            loss = (wt * out).sum()
            loss.backward()
            for k, p in vl.named_parameters():
                g["grad_%s_%s_%s" % (tag, size or 0, k)] = p.grad.detach().numpy().copy()
            g["loss_%s_%s" % (tag, size or 0)] = float(loss)
    np.savez_compressed(os.path.join(HERE, "est_grad.npz"), **g)
    print("wrote est_grad.npz", sorted(g))


if __name__ == "__main__":
    main()
