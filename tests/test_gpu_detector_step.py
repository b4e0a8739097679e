"""GPU: the parameter update (csrc/evrep_step.hip through evrep_train_step / evrep_ema_update and detector_step's SGD,
GradScaler, ModelEMA and TrainStep) against the host statements (detector_step.step_host).  Everything is bit for bit: the
kernel and the mirror run the same float32 statements in the same order, each rounded on its own.

Every array the kernels touch is carved from tests/guarded.py's Arena, and its guard bands are checked after every call.  The
raw-entry tests place the first element of p, g, buf and ema of one tensor 0, 4, 8 and 12 bytes past a 16-byte boundary, each at
a different offset, inside a region three floats longer than the tensor: the floats of slack in front of and behind the
tensor are compared too, since a 16-byte store that starts one element early stays inside the guard's region.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal
import detector_step_cases as cases
from guarded import Arena

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32
GROUPS = ((0.01, 0.9, 5e-4), (0.02, 0.8, 0.0), (0.1, 0.5, 1e-3))       # three groups, one of them without weight decay
AMP = (2.0, 0.5)


def _ds():
    from event_representation_study_amd import detector_step
    return detector_step


def _lib():
    from event_representation_study_amd import _lib
    return _lib


def _sizes():
    c = _lib().STEP_CHUNK
    #       (n, kind): the last tensor has a gradient and ends in a chunk of five elements; the one of 0 elements has a row and no chunk
    return [(7, "no_grad"), (c + 3, "ema_only"), (0, "grad"), (1, "grad"), (3, "grad"), (c - 1, "grad"), (c, "grad"), (c + 1, "grad"), (2 * c + 5, "grad")]


class Rig:
    """Tensors of the sizes above in one table, on the device and mirrored on the host; `step` runs evrep_train_step and
    step_host on the same inputs and compares every array, every float of slack, the state words and the guard bands."""

    def __init__(self, seed, ema=True, scaler=True, init_scale=256.0):
        ds, lib = _ds(), _lib()
        self.ds, self.lib, self.rng = ds, lib, np.random.default_rng(seed)
        self.arena = Arena(DEV, seed)
        self.ema, self.scaler = ema, scaler
        self.rows, self.raw = [], []
        for i, (n, kind) in enumerate(_sizes()):
            row = dict(n=n, kind=kind, group=i % 3, dev={}, host={}, addr={})
            row["flags"] = (ds.HAS_GRAD if kind == "grad" else 0) | (ds.HAS_EMA if ema else 0) | (ds.EMA_ONLY if kind == "ema_only" else 0)
            for j, what in enumerate(("p", "g", "buf", "ema")):
                if (what in ("g", "buf") and kind != "grad") or (what == "ema" and not ema):
                    continue
                off = (i + j) % 4                                        # 0, 4, 8, 12 bytes past a 16-byte boundary, all four apart
                raw = self.arena.carve_shape((n + 3,), torch.float32, name="%s%d" % (what, i), align=16)
                view = raw[off:off + n]
                row["addr"][what] = raw.data_ptr() + 4 * off               # (an empty view has no address of its own)
                assert row["addr"][what] % 16 == 4 * off and (n == 0 or view.data_ptr() == row["addr"][what])
                if what != "buf":                                        # a buffer starts as the arena's garbage: not read before it is written
                    view.copy_(torch.from_numpy(self.rng.normal(size=n).astype(F32)))
                row["dev"][what], row["host"][what] = view, view.cpu().numpy().copy()
                self.raw.append((raw, off, n, "%s%d" % (what, i)))
            self.rows.append(row)
        self.rows = [r for r in self.rows if "ema" in r["dev"] or r["kind"] == "grad"]    # without EMA the two others have nothing to do
        self.amp = self.arena.carve_shape((lib.STEP_AMP_WORDS,), torch.int32, name="amp", align=4) if scaler else None
        self.applied = self.arena.carve_shape((1,), torch.int32, name="applied", align=4)
        self.applied.zero_()
        self.state = ds.new_state(scale=init_scale if scaler else 1.0)
        if scaler:
            self.amp.copy_(torch.tensor([0, int(np.float32(init_scale).view(np.int32)), 0], dtype=torch.int32))
        self.hyper = self.arena.carve_shape((lib.STEP_HYPER_EMA + 3 * len(GROUPS),), torch.float32, name="hyper", align=4)
        tens = np.zeros(len(self.rows), dtype=ds.TENSOR_DTYPE)
        chunks = []
        for i, r in enumerate(self.rows):
            ptr = lambda k: r["addr"].get(k, 0)
            tens[i] = (ptr("p"), ptr("g"), ptr("buf"), ptr("ema"), r["n"], r["group"], r["flags"])
            for first in range(0, r["n"], lib.STEP_CHUNK):
                chunks.append((first, i, min(lib.STEP_CHUNK, r["n"] - first)))
        chunks = np.array(chunks, dtype=ds.CHUNK_DTYPE)
        self.n_tensors, self.n_chunks = len(tens), len(chunks)
        up = lambda a, name: self.arena.carve_like(torch.from_numpy(np.frombuffer(a.tobytes(), dtype=np.uint8).copy()), name=name)
        self.tensors_dev, self.chunks_dev = up(tens, "tensors"), up(chunks, "chunks")

    def grads(self, scale=64.0):
        return {i: (self.rng.normal(size=r["n"]) * scale).astype(F32) for i, r in enumerate(self.rows) if r["kind"] == "grad"}

    def step(self, grads, decay=0.37, interval=2000, zero_grad=True, groups=GROUPS):
        ds, lib = self.ds, self.lib
        hyper = ds.hyper_row(groups, decay if self.ema else None)
        self.hyper.copy_(torch.from_numpy(hyper))
        for i, g in grads.items():
            self.rows[i]["dev"]["g"].copy_(torch.from_numpy(g))
            self.rows[i]["host"]["g"] = g.copy()
        for r in self.rows:                                              # a forward pass leaves new statistics in an EMA-only entry
            if r["kind"] == "ema_only":
                r["host"]["p"] = self.rng.normal(size=r["n"]).astype(F32)
                r["dev"]["p"].copy_(torch.from_numpy(r["host"]["p"]))
        before = [raw.clone() for raw, _, _, _ in self.raw]
        flags = ds.ZERO_GRAD if zero_grad else 0
        vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        lib.api().evrep_train_step(vp(self.tensors_dev), self.n_tensors, vp(self.chunks_dev), self.n_chunks, vp(self.hyper), len(groups),
                                   vp(self.amp), vp(self.applied), AMP[0], AMP[1], interval, flags, None)
        torch.cuda.synchronize()
        self.arena.check()
        self.arena.check_inputs()                                        # the two tables are only read
        for (raw, off, n, name), b in zip(self.raw, before):
            assert torch.equal(raw[:off].view(torch.int32), b[:off].view(torch.int32)), name + ": slack in front"
            assert torch.equal(raw[off + n:].view(torch.int32), b[off + n:].view(torch.int32)), name + ": slack behind"
        host_rows = [dict(p=r["host"]["p"], g=r["host"].get("g"), buf=r["host"].get("buf"), ema=r["host"].get("ema"), group=r["group"],
                          flags=r["flags"]) for r in self.rows]
        g_in = {i: r["host"]["g"].copy() for i, r in enumerate(self.rows) if r["kind"] == "grad"}
        ds.step_host(host_rows, hyper, self.state, (AMP[0], AMP[1], interval) if self.scaler else None, zero_grad)
        for i, r in enumerate(self.rows):
            for what, view in r["dev"].items():
                assert_bit_equal(view.cpu().numpy(), r["host"][what], "%s of tensor %d (n = %d, %s)" % (what, i, r["n"], r["kind"]))
            if r["kind"] == "grad":
                want = np.zeros(r["n"], F32) if zero_grad else g_in[i]
                assert_bit_equal(r["dev"]["g"].cpu().numpy(), want, "g of tensor %d after the step" % i)
        if self.scaler:
            amp = self.amp.cpu().numpy()
            assert amp[0] == 0 and amp[1] == np.float32(self.state["scale"]).view(np.int32) and amp[2] == self.state["tracker"], \
                (amp, self.state)
        assert int(self.applied.item()) == self.state["applied_steps"]
        return self.state


def _poison_last(rig, grads, value):
    last = max(grads)
    assert last == len(rig.rows) - 1 and rig.rows[last]["n"] % rig.lib.STEP_CHUNK == 5
    grads[last][-1] = value                                              # the last element of the last chunk of the last tensor
    return grads


def test_every_shape_and_offset_in_one_table():
    """0, 1, 3, C - 1, C, C + 1 and 2C + 5 elements, a tensor without a gradient and an EMA-only buffer, three groups, all four
    offsets: the first step clones d (with -0.0 gradients among them), the second and third use the buffers, the fourth finds a
    single NaN in the very last element and is skipped with a backoff, the fifth goes on."""
    rig = Rig(1)
    g = rig.grads()
    for v in g.values():
        v[::3] = -0.0                                                    # d = -0.0 where the group has no weight decay: buf must be -0.0
    before_buf = {i: r["dev"]["buf"].clone() for i, r in enumerate(rig.rows) if r["kind"] == "grad" and r["n"] > 0}
    st = rig.step(g)
    assert st["applied_steps"] == 1 and st["tracker"] == 1
    nowd = [i for i, r in enumerate(rig.rows) if r["kind"] == "grad" and GROUPS[r["group"]][2] == 0.0]
    assert nowd and all(np.signbit(rig.rows[i]["host"]["buf"][::3]).all() for i in nowd)
    assert all(not torch.equal(before_buf[i].view(torch.int32), rig.rows[i]["dev"]["buf"].view(torch.int32)) for i in before_buf)
    rig.step(rig.grads(), decay=0.61)
    rig.step(rig.grads(), decay=0.83, groups=((0.03, 0.7, 1e-4), (0.0, 0.0, 0.0), (0.05, 0.9, 0.0)))   # warm-up rewrites; momentum 0 in one group
    p3 = [r["host"]["p"].copy() for r in rig.rows]
    st = rig.step(_poison_last(rig, rig.grads(), np.nan), decay=0.9)
    assert st["applied_steps"] == 3 and st["scale"] == 128.0 and st["tracker"] == 0
    assert all(np.array_equal(a, r["host"]["p"]) for a, r in zip(p3, rig.rows) if r["kind"] == "grad")
    st = rig.step(rig.grads(), decay=0.95)
    assert st["applied_steps"] == 4 and st["tracker"] == 1


def test_overflow_on_the_very_first_step_then_a_step_that_clones():
    rig = Rig(2)
    garbage = {i: r["dev"]["buf"].clone() for i, r in enumerate(rig.rows) if r["kind"] == "grad"}
    st = rig.step(_poison_last(rig, rig.grads(), np.inf))
    assert st["applied_steps"] == 0 and st["scale"] == 128.0
    assert all(torch.equal(garbage[i].view(torch.int32), rig.rows[i]["dev"]["buf"].view(torch.int32)) for i in garbage)   # left uninitialised
    g = rig.grads()
    st = rig.step(g)
    assert st["applied_steps"] == 1
    st = rig.step(_poison_last(rig, rig.grads(), -np.inf))
    assert st["applied_steps"] == 1 and st["scale"] == 64.0


def test_growth_at_interval_two():
    rig = Rig(3)
    scales = [float(rig.step(rig.grads(), interval=2)["scale"]) for _ in range(4)]
    assert scales == [256.0, 512.0, 512.0, 1024.0] and rig.state["tracker"] == 0


def test_without_a_scaler():
    rig = Rig(4, scaler=False)
    for _ in range(2):
        rig.step(rig.grads(scale=1.0))
    assert rig.state["applied_steps"] == 2


def test_without_an_ema():
    rig = Rig(5, ema=False)
    for _ in range(2):
        rig.step(rig.grads())


def test_gradients_are_kept_without_zero_grad():
    rig = Rig(6)
    for _ in range(2):
        rig.step(rig.grads(), zero_grad=False)
    rig.step(_poison_last(rig, rig.grads(), np.nan), zero_grad=False)    # a skipped step keeps them too, NaN included


# ------------------------------------------------------------------------------------------------------------ the module's route
@pytest.fixture(scope="module")
def hosts():
    return {name: cases.run_host(cases.build(name)) for name in cases.GOLDEN}


def _same(got, host, name):
    written = ~np.isnan(host["buf"])
    for k in ("p", "ema", "scale", "tracker", "applied"):
        assert_bit_equal(got[k], host[k], "%s: %s" % (name, k))
    assert_bit_equal(got["buf"][written], host["buf"][written], name + ": buf")


@pytest.mark.parametrize("name", list(cases.GOLDEN))
def test_golden_cases_end_to_end(hosts, name):
    """SGD + GradScaler + ModelEMA + TrainStep on CUDA tensors, every tensor carved from an arena, over all recorded steps."""
    got, objs = cases.run_module(cases.build(name), DEV, arena=Arena(DEV, 7))
    _same(got, hosts[name], name)
    assert objs["step"].table_uploads == 1


def test_two_identical_runs_give_equal_bits():
    c = cases.build("overflow_mid")
    a, _ = cases.run_module(c, DEV)
    b, _ = cases.run_module(c, DEV)
    for k in a:
        assert_bit_equal(a[k], b[k], k)


def test_model_ema_update_alone():
    ds = _ds()
    arena = Arena(DEV, 8)
    m = cases.rehome(cases.model(21).to(DEV), arena)
    ema = ds.ModelEMA(m, decay=0.999, updates=3)
    cases.rehome(ema.ema, arena)
    e = {k: v.cpu().numpy().copy() for k, v in ema.ema.state_dict().items()}
    rng = np.random.default_rng(9)
    for t in range(3):
        with torch.no_grad():
            for v in m.state_dict().values():
                if v.dtype.is_floating_point:
                    v.copy_(torch.from_numpy(rng.normal(size=tuple(v.shape)).astype(F32)))
            m.bn.num_batches_tracked += 1
        ema.update(m)
        torch.cuda.synchronize()
        arena.check()
        hyper = ds.hyper_row((), ema.decay(4 + t))
        for k, v in ema.ema.state_dict().items():
            if v.dtype.is_floating_point:
                ds.step_host([dict(p=m.state_dict()[k].cpu().numpy(), ema=e[k])], hyper, None, ema_only=True)
            assert_bit_equal(v.cpu().numpy(), e[k], "%s after update %d" % (k, t))
    assert ema.updates == 6 and ema.table_uploads == 1 and int(ema.ema.bn.num_batches_tracked) == 0


def test_an_empty_parameter_contributes_no_chunk():
    ds = _ds()
    empty, p = torch.nn.Parameter(torch.empty(0, device=DEV)), torch.nn.Parameter(torch.tensor([1.0, -2.0], device=DEV))
    opt = ds.SGD([empty, p], lr=0.5, momentum=0.5, nesterov=True)
    empty.grad, p.grad = torch.empty(0, device=DEV), torch.tensor([2.0, 2.0], device=DEV)
    opt.step()
    assert p.detach().cpu().tolist() == [-0.5, -3.5] and p.grad.cpu().tolist() == [0.0, 0.0] and opt._table.n_chunks == 1
    only = ds.SGD([torch.nn.Parameter(torch.empty(0, device=DEV))], lr=0.5)
    only.param_groups[0]["params"][0].grad = torch.empty(0, device=DEV)
    only.step()                                                          # no chunk at all: the finish launch alone
    assert only.applied_steps() == 1


def test_a_captured_step_replays_the_eager_step(hosts):
    """No host read: TrainStep.__call__ is captured into a graph (the hyper row uploaded outside the capture), and the replay
    equals the eager step bit for bit.  The captured launch is the optimizer's first, so nothing it needs may be made by it:
    an allocation inside the capture would run again on every replay and set applied_steps back to 0."""
    c = cases.build("shipped")
    results = []
    for captured in (False, True):
        m = cases.model(c["seed"]).to(DEV)
        ds = _ds()
        opt = ds.build_optimizer(cases.cfg(), m)
        step = ds.TrainStep(opt, ds.GradScaler(init_scale=c["scaler"][0]), ds.ModelEMA(m))
        params = dict(m.named_parameters())
        grads = {k: torch.zeros_like(p) for k, p in params.items()}
        for k, p in params.items():
            p.grad = grads[k]
        graph = None
        for t in range(c["steps"]):
            with torch.no_grad():
                for k in cases.STATS:
                    dict(m.named_buffers())[k].copy_(torch.from_numpy(c["stats"][t][k]))
                for k, g in grads.items():
                    g.copy_(torch.from_numpy(c["grads"][t][k]))
            if not captured:
                step(m)
                continue
            step.refresh(m)                                              # the tables, the hyper row AND the state words: the first
            #                                                              launch of all is the captured one
            if graph is None:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    step(m)
            graph.replay()
        torch.cuda.synchronize()
        results.append((cases.flat({k: p.detach().cpu().numpy() for k, p in params.items()}, cases.param_keys(m)),
                        cases.flat({k: v.cpu().numpy() for k, v in step.ema.ema.state_dict().items()}, cases.ema_keys(m)),
                        opt.applied_steps(), step.scaler.get_scale(), step.ema.updates))
    for a, b in zip(*results):
        assert_bit_equal(np.asarray(a), np.asarray(b), "captured against eager")
    assert_bit_equal(results[0][0], hosts["shipped"]["p"][-1], "eager against the host")
    assert_bit_equal(results[0][1], hosts["shipped"]["ema"][-1], "eager EMA against the host")


def test_driven_by_torchs_own_grad_scaler(hosts):
    """A plain torch.amp.GradScaler hands found_inf and the scale over through _step_supports_amp_scaling; without an overflow
    the parameters and the EMA equal the fused route's."""
    ds = _ds()
    c = cases.build("shipped")
    m = cases.model(c["seed"]).to(DEV)
    opt, ema = ds.build_optimizer(cases.cfg(), m), ds.ModelEMA(m)
    scaler = torch.amp.GradScaler("cuda", init_scale=c["scaler"][0], growth_interval=c["scaler"][1])
    params = dict(m.named_parameters())
    for t in range(c["steps"]):
        with torch.no_grad():
            for k in cases.STATS:
                dict(m.named_buffers())[k].copy_(torch.from_numpy(c["stats"][t][k]))
        for k, p in params.items():
            p.grad = torch.from_numpy(c["grads"][t][k]).to(DEV)
        scaler.scale(torch.zeros((), device=DEV))
        scaler.step(opt)
        scaler.update()
        ema.update(m)
    assert_bit_equal(cases.flat({k: p.detach().cpu().numpy() for k, p in params.items()}, cases.param_keys(m)), hosts["shipped"]["p"][-1], "p")
    assert_bit_equal(cases.flat({k: v.cpu().numpy() for k, v in ema.ema.state_dict().items()}, cases.ema_keys(m)),
                     hosts["shipped"]["ema"][-1], "ema")
    assert scaler.get_scale() == c["scaler"][0] and opt.applied_steps() == c["steps"]
