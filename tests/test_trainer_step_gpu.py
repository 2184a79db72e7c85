"""The optimizer step on the MI355X (csrc/optim.hip, training/optim.py, training/trainer.py): gradient norm + clip, Adam and EMA against
torch.optim.Adam + clip_grad_norm_ in fp64, the skips decided on the device, graph replays, `GraphedTrainStep(optimizer=)` and `Trainer`.

Shapes (the smallest at which the kernels can go wrong): tensors of 1, 3, 4, 5, 255, 256, 257, 4096, 4097 and 70001 values around the
16-byte body and the 4096-value chunk, one of zero values, one without a gradient, three views into flat buffers at element offsets 1, 2
and 3 (the third with a gradient whose address disagrees modulo 16: the 4-byte path); the "big" case adds one tensor of 1 100 003 values,
so that the finish workgroup (256 lanes) adds more than one partial per lane.  Seeded inputs: 0.1 randn parameters, gradients 0.02 randn
on even and 0.002 randn on odd steps, max_grad_norm 1: in the small case the norm alternates between ~5.8 and ~0.58 (clipping active and
inactive in turn); in the big case it is active throughout.

Bounds.  Adam (and the EMA): 2 x the worst absolute error of torch.optim.Adam(fused=True) + clip_grad_norm_ in fp32 on the same GPU and
inputs against the same fp64 run -- the two fp32 chains differ in rounding order only.  Norm: 2 x the relative error of PyTorch's fp32
clip_grad_norm_, floor 2^-22 (the result is stored as fp32: half an ulp is 2^-24 ... 2^-25 relative, the fp32 partials of 4096 squares add
a few more).  Measured figures are printed and recorded under `tests` in profiles/trainer_step.json (NS2_RECORD_DIR names another directory to write to)."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from naturalspeech2_pytorch_amd import Model, NaturalSpeech2, ops, training  # noqa: E402
from naturalspeech2_pytorch_amd.training import HipAdam, Trainer  # noqa: E402
from tests.golden.gen import make_input, make_weights  # noqa: E402
from tests.trainer_ref64 import Ref64  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SIZES = [1, 3, 4, 5, 255, 256, 257, 4096, 4097, 70001, 0, 33]
I257, INOGRAD = SIZES.index(257), SIZES.index(33)
VIEWS = [(1, 37), (64 + 2, 4100), (8192 + 3, 9)]            # (element offset in the flat buffer, values)
NSTEPS = 7


def _record(key, value):
    """merge one figure into the `tests` entry of profiles/trainer_step.json, or of the copy under $NS2_RECORD_DIR where only that travels"""
    tracked = os.path.join(ROOT, "profiles", "trainer_step.json")
    out = os.path.join(os.environ["NS2_RECORD_DIR"], "trainer_step.json") if os.environ.get("NS2_RECORD_DIR") else tracked
    cur = {}
    for path in (tracked, out):
        try:
            with open(path) as f:
                cur.update(json.load(f))
        except Exception:
            pass
    cur.setdefault("tests", {})[key] = value
    try:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(cur, f, indent=1, sort_keys=True)
    except OSError:
        pass


class Case:
    """seeded CPU inputs of one set of tensors: p0[i], grads[s][i] (None: no gradient)"""

    def __init__(self, big):
        g = torch.Generator().manual_seed(1234)
        self.sizes = SIZES + [n for _, n in VIEWS] + ([1_100_003] if big else [])
        self.nview0 = len(SIZES)
        self.p0 = [0.1 * torch.randn(n, generator=g) for n in self.sizes]
        self.grads = [[None if i == INOGRAD else (0.02 if s % 2 == 0 else 0.002) * torch.randn(n, generator=g)
                       for i, n in enumerate(self.sizes)] for s in range(NSTEPS)]

    def on_gpu(self):
        """fresh parameters and gradient buffers on the GPU: (params, gbufs); the views live in flat buffers"""
        flat_p, flat_g = torch.zeros(8300, device=DEV), torch.zeros(8300, device=DEV)
        ps, gs = [], []
        for i, p0 in enumerate(self.p0):
            k = i - self.nview0
            if 0 <= k < len(VIEWS):
                off, n = VIEWS[k]
                flat_p[off:off + n] = p0.to(DEV)
                ps.append(flat_p[off:off + n].detach().requires_grad_(True))
                gs.append(flat_g[off:off + n] if k < 2 else torch.zeros(n, device=DEV))     # k == 2: the gradient is 16-byte aligned, the parameter is not
                assert ps[-1].data_ptr() % 16 == 4 * (off % 4) and (gs[-1].data_ptr() % 16 == ps[-1].data_ptr() % 16) == (k < 2)
            else:
                ps.append(p0.to(DEV).clone().requires_grad_(True))
                gs.append(None if i == INOGRAD else torch.zeros_like(ps[-1]))
        return ps, gs

    def load_grads(self, gbufs, s, poison=None):
        for i, (b, g) in enumerate(zip(gbufs, self.grads[s])):
            if b is not None:
                b.copy_(g.to(DEV))
        if poison is not None:
            gbufs[I257][-1] = poison


def _state(opt, ps):
    out = {"p": [p.detach().clone() for p in ps], "m": [t.clone() for t in opt._m], "v": [t.clone() for t in opt._v],
           "t": opt.steps_taken.clone()}
    if opt.use_ema:
        out["ema"] = [t.clone() for t in opt.ema_parameters()]
    return out


def _same_bits(a, b):
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for i, (x, y) in enumerate(zip(xs, ys)):
            if not torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y):
                return f"{k}[{i}]"
    return None


def run_hip(case, steps, max_grad_norm=1.0, graph=False, poison=None, before_step=None, keep_states=False, skip_steps=(), **kw):
    """HipAdam over fresh GPU copies of the case: returns the final state, the per-step device scalars and (keep_states) every state.
    poison = {step: value}; before_step(opt, s) runs in front of step s; skip_steps: gradient steps of the case left out."""
    ps, gbufs = case.on_gpu()
    opt = HipAdam(ps, max_grad_norm=max_grad_norm, **kw)
    opt.bind(ps, gbufs)
    opt.prepare()
    g = None
    if graph:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            opt.step()
    norms, skipped, states = [], [], []
    for s in range(steps):
        if s in skip_steps:
            continue
        case.load_grads(gbufs, s, (poison or {}).get(s))
        if before_step is not None:
            before_step(opt, s)
        g.replay() if graph else opt.step()
        norms.append(opt.grad_norm.clone())
        skipped.append(opt.skipped.clone())
        if keep_states:
            states.append(_state(opt, ps))
    torch.cuda.synchronize()
    return {"state": _state(opt, ps), "norms": [float(n) for n in norms], "skipped": [int(k) for k in skipped], "states": states,
            "opt": opt, "ps": ps, "gbufs": gbufs}


class Refs:
    """computed once per case and left unchanged: torch.optim.Adam + clip_grad_norm_ in fp64 (CPU) and fused in fp32 (GPU), 6 steps"""

    def __init__(self, big):
        self.case = c = Case(big)
        p64 = [torch.nn.Parameter(p.double()) for p in c.p0]
        a64 = torch.optim.Adam(p64, lr=1e-4, betas=(0.9, 0.99), eps=1e-8)
        p32, g32 = c.on_gpu()
        a32 = torch.optim.Adam(p32, lr=1e-4, betas=(0.9, 0.99), eps=1e-8, fused=True)
        self.norm64, self.norm32 = [], []
        for s in range(6):
            for p, g in zip(p64, c.grads[s]):
                p.grad = None if g is None else g.double()
            self.norm64.append(float(torch.nn.utils.clip_grad_norm_(p64, 1.0)))
            a64.step()
            c.load_grads(g32, s)
            for p, g in zip(p32, g32):
                p.grad = g
            self.norm32.append(float(torch.nn.utils.clip_grad_norm_(p32, 1.0)))      # (scales g32 in place: reloaded every step)
            a32.step()
        live = [i for i in range(len(p64)) if i != INOGRAD and c.sizes[i] > 0]
        self.p = [p.detach() for p in p64]
        self.m = [a64.state[p64[i]]["exp_avg"] if i in live else torch.zeros_like(p64[i]) for i in range(len(p64))]
        self.v = [a64.state[p64[i]]["exp_avg_sq"] if i in live else torch.zeros_like(p64[i]) for i in range(len(p64))]
        err = lambda xs, ys: max(float((x.detach().double().cpu() - y).abs().max()) for x, y in zip(xs, ys) if y.numel())   # noqa: E731
        self.err = err
        self.fused_err = {"p": err(p32, self.p),
                          "m": err([a32.state[p32[i]]["exp_avg"] if i in live else torch.zeros_like(p32[i]) for i in range(len(p32))], self.m),
                          "v": err([a32.state[p32[i]]["exp_avg_sq"] if i in live else torch.zeros_like(p32[i]) for i in range(len(p32))], self.v)}
        self.norm32_err = max(abs(a - b) / b for a, b in zip(self.norm32, self.norm64))


_REFS = {}


@pytest.fixture(params=[False, True], ids=["small", "big"])
def refs(request):
    if request.param not in _REFS:
        _REFS[request.param] = Refs(request.param)
    return _REFS[request.param]


@pytest.fixture
def small():
    if False not in _REFS:
        _REFS[False] = Refs(False)
    return _REFS[False]


# =============================================================================================== 1. Adam parity
def test_adam_matches_fp64_within_twice_fused_adams_error(refs):
    r = run_hip(refs.case, 6)
    st = r["state"]
    ours = {k: refs.err(st[k], getattr(refs, k)) for k in ("p", "m", "v")}
    big = len(refs.case.sizes) > len(SIZES) + len(VIEWS)
    print(f"\nadam parity ({'big' if big else 'small'}): worst abs error vs fp64  ours {ours}  fused fp32 {refs.fused_err}")
    _record(f"adam_parity_{'big' if big else 'small'}", {"hip_abs_err": ours, "torch_fused_fp32_abs_err": refs.fused_err, "bound": "2 x fused"})
    assert int(st["t"]) == 6 and r["skipped"] == [0] * 6
    assert torch.equal(st["p"][INOGRAD].cpu(), refs.case.p0[INOGRAD]) and not st["m"][INOGRAD].any()      # no gradient: untouched
    for k in ("p", "m", "v"):
        assert ours[k] <= 2 * refs.fused_err[k], (k, ours[k], refs.fused_err[k])


def test_clip_inactive_steps_are_bit_identical_to_no_clipping(small):
    c = small.case
    assert [n > 1.0 for n in small.norm64] == [True, False] * 3           # clipping active and inactive in turn
    a = run_hip(c, 6, keep_states=True)
    ps, gbufs = c.on_gpu()
    b = HipAdam(ps, max_grad_norm=None)
    b.bind(ps, gbufs)
    b.prepare()
    for s in (1, 3, 5):
        prev = a["states"][s - 1]
        for dst, src in zip(ps + b._m + b._v, prev["p"] + prev["m"] + prev["v"]):
            dst.detach().copy_(src)
        b.steps_taken.copy_(prev["t"])
        c.load_grads(gbufs, s)
        b.step()
        assert _same_bits(a["states"][s], _state(b, ps)) is None, s
    # ... and an active step is not (the comparison can tell)
    prev = a["states"][1]
    for dst, src in zip(ps + b._m + b._v, prev["p"] + prev["m"] + prev["v"]):
        dst.detach().copy_(src)
    b.steps_taken.copy_(prev["t"])
    c.load_grads(gbufs, 2)
    b.step()
    assert _same_bits(a["states"][2], _state(b, ps)) is not None


# =============================================================================================== 2. norm
def test_grad_norm_against_fp64(refs):
    r = run_hip(refs.case, 6)
    ours = max(abs(a - b) / b for a, b in zip(r["norms"], refs.norm64))
    bound = max(2 * refs.norm32_err, 2.0 ** -22)
    print(f"\ngrad_norm worst relative error vs fp64: ours {ours:.3e}  torch fp32 clip_grad_norm_ {refs.norm32_err:.3e}  bound {bound:.3e}")
    _record(f"grad_norm_{len(refs.case.sizes)}_tensors", {"hip_rel_err": ours, "torch_fp32_rel_err": refs.norm32_err, "bound": bound})
    assert ours <= bound


# =============================================================================================== 3. reproducibility
def test_two_runs_and_a_graph_replay_give_the_same_bits(refs):
    a = run_hip(refs.case, 6, ema=True, ema_update_every=2)
    b = run_hip(refs.case, 6, ema=True, ema_update_every=2)
    g = run_hip(refs.case, 6, ema=True, ema_update_every=2, graph=True)
    assert _same_bits(a["state"], b["state"]) is None and a["norms"] == b["norms"]
    assert _same_bits(a["state"], g["state"]) is None and a["norms"] == g["norms"]
    assert int(a["state"]["t"]) == 6


# =============================================================================================== 4. non-finite skip
@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_a_non_finite_gradient_skips_the_step_and_leaves_no_trace(small, bad):
    c = small.case
    x = run_hip(c, 4, poison={2: bad}, keep_states=True, ema=True, ema_update_every=2)
    assert x["skipped"] == [0, 0, 1, 0]
    assert _same_bits(x["states"][1], x["states"][2]) is None            # p, m, v, ema and the step count keep their bits
    assert int(x["states"][2]["t"]) == 2 and int(x["state"]["t"]) == 3
    y = run_hip(c, 4, skip_steps=(2,), ema=True, ema_update_every=2)      # the run that never saw the bad step
    assert _same_bits(x["state"], y["state"]) is None


# =============================================================================================== 5. range skip
def _clamp_once():
    x = torch.zeros(32, 32, device=DEV)
    x[3, 5] = 1e5                                                         # beyond 65504: the conversion clamps and counts (test_range_guard_gpu.py)
    ops.relu_split(x, precision=4)


def test_a_range_counter_that_moved_since_mark_skips_the_step(small):
    c = small.case

    def marked_then_clamp(opt, s):
        opt.mark()
        if s == 1:
            _clamp_once()

    a = run_hip(c, 3, before_step=marked_then_clamp)
    assert a["skipped"] == [0, 1, 0] and int(a["state"]["t"]) == 2
    b = run_hip(c, 3, before_step=lambda opt, s: _clamp_once() if s == 1 else None)      # the same sequence, never marked
    assert b["skipped"] == [0, 0, 0] and int(b["state"]["t"]) == 3
    y = run_hip(c, 3, skip_steps=(1,))
    assert _same_bits(a["state"], y["state"]) is None


# =============================================================================================== 6. EMA
def test_ema_every_third_step_with_a_decay_rewritten_between_steps(small):
    c = small.case
    ref = Ref64(c.p0, max_grad_norm=1.0, ema=True, update_every=3)
    for s in range(7):
        assert ref.step(c.grads[s], ema_decay=0.9 if s >= 5 else 0.995)

    def rewrite(opt, s):
        if s == 5:
            opt.ema_decay.fill_(0.9)

    r = run_hip(c, 7, ema=True, ema_update_every=3, before_step=rewrite, keep_states=True)
    err = small.err(r["state"]["ema"], ref.ema)
    perr = small.err(r["state"]["p"], ref.p)
    print(f"\nema worst abs error vs fp64 {err:.3e} (parameters {perr:.3e}); bound 2 x fused Adam's {small.fused_err['p']:.3e}")
    _record("ema_small", {"hip_ema_abs_err": err, "hip_param_abs_err": perr, "bound": 2 * small.fused_err["p"]})
    assert err <= 2 * small.fused_err["p"]
    for s in range(1, 7):                                                 # due after steps 3 and 6 (s = 2, 5); bits kept otherwise
        moved = _same_bits({"ema": r["states"][s - 1]["ema"]}, {"ema": r["states"][s]["ema"]}) is not None
        assert moved == (s in (2, 5)), s
    const = run_hip(c, 7, ema=True, ema_update_every=3)                   # the rewritten decay made a difference
    assert _same_bits({"ema": const["state"]["ema"]}, {"ema": r["state"]["ema"]}) is not None
    assert _same_bits({"p": const["state"]["p"]}, {"p": r["state"]["p"]}) is None


# =============================================================================================== 7. lr under replay
def test_lr_rewritten_between_replays_is_honoured(small):
    c = small.case
    lrs = [1e-4, 1e-4, 5e-4, 5e-4, 2e-5, 2e-5]

    def rewrite(opt, s):
        opt.lr.fill_(lrs[s])

    g = run_hip(c, 6, graph=True, before_step=rewrite)
    e = run_hip(c, 6, before_step=rewrite)
    assert _same_bits(g["state"], e["state"]) is None
    ref = Ref64(c.p0, max_grad_norm=1.0)
    for s in range(6):
        ref.step(c.grads[s], lr=float(torch.tensor(lrs[s], dtype=torch.float32)))
    err = small.err(g["state"]["p"], ref.p)
    bound = 2 * small.fused_err["p"] * max(lrs) / 1e-4                    # the yardstick was measured at lr 1e-4; an update's rounding scales with lr
    print(f"\nlr under replay: worst abs error vs fp64 {err:.3e}  bound {bound:.3e}")
    assert err <= bound
    assert small.err(run_hip(c, 6, graph=True)["state"]["p"], ref.p) > 1e-5      # a constant lr is far from it


# =============================================================================================== 8. GraphedTrainStep(optimizer=)
def _model(tprec, seed=71):
    m = Model(dim=64, depth=1)
    m.load_state_dict(make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed))
    m = m.to(DEV).train()
    m.train_backend, m.train_precision = "hip", tprec
    return m, NaturalSpeech2(m, codec=None, target_sample_hz=24000, timesteps=2).to(DEV)


def _batch(s):
    mk = lambda name, shape, **k: make_input(name, shape, seed=s, **k).to(DEV)    # noqa: E731
    return mk("audio", (2, 96, 64)), mk("times", (2,), uniform=True), mk("noise", (2, 96, 64))


@pytest.mark.parametrize("tprec", ["exact", "mixed"])
def test_graphed_train_step_with_the_optimizer_inside(tprec):
    batches = [_batch(80 + i) for i in range(5)]
    kw = dict(lr=1e-4, max_grad_norm=1.0, ema=True, ema_update_every=2)      # lr: HipAdam's and the Trainer's default

    def eager(make_opt, clip):
        m, d = _model(tprec)
        opt = make_opt(m)
        losses = []
        for a, t, z in batches:
            for p in m.parameters():
                p.grad = None
            if isinstance(opt, HipAdam):
                opt.mark()
            loss = d(a, times=t, noise=z)
            loss.backward()
            if clip:
                torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
            opt.step()
            losses.append(loss.detach().clone())
        return m, opt, [float(x) for x in losses]

    m, d = _model(tprec)
    opt = HipAdam(m.parameters(), **kw)
    opt.init_state()
    before = _state(opt, list(m.parameters()))
    step = training.GraphedTrainStep(lambda a, t, z: d(a, times=t, noise=z), batches[0], m, optimizer=opt)
    torch.cuda.synchronize()
    assert _same_bits(before, _state(opt, list(m.parameters()))) is None, "construction moved a parameter or optimizer state"
    losses = [float(step(*b).detach().clone()) for b in batches]
    assert int(opt.steps_taken) == 5 and int(opt.skipped) == 0

    m_e, opt_e, losses_e = eager(lambda mm: HipAdam(mm.parameters(), **kw), clip=False)
    assert losses == losses_e
    assert _same_bits(_state(opt, list(m.parameters())), _state(opt_e, list(m_e.parameters()))) is None
    assert any(not torch.equal(a, b) for a, b in zip(before["p"], [p.detach() for p in m.parameters()]))

    tk = dict(lr=1e-4, betas=(0.9, 0.99), eps=1e-8)
    _, _, l_fused = eager(lambda mm: torch.optim.Adam(mm.parameters(), fused=True, **tk), clip=True)
    _, _, l_foreach = eager(lambda mm: torch.optim.Adam(mm.parameters(), foreach=True, **tk), clip=True)
    rel = lambda xs, ys: max(abs(x - y) / abs(y) for x, y in zip(xs, ys))   # noqa: E731
    yard, ours = rel(l_fused, l_foreach), rel(losses, l_fused)
    bound = max(4 * yard, 1e-6)
    print(f"\n{tprec}: loss trajectory  ours vs fused {ours:.3e}   fused vs foreach {yard:.3e}   bound {bound:.3e}\n  ours {losses}\n  fused {l_fused}")
    _record(f"graphed_step_{tprec}", {"loss_rel_gap_hip_vs_fused": ours, "loss_rel_gap_fused_vs_foreach": yard, "bound": bound, "losses": losses})
    assert ours <= bound


# =============================================================================================== 9. Trainer
def test_trainer_runs_saves_and_restores(tmp_path):
    m, d = _model("exact", seed=5)
    data = [make_input("audio", (2, 96, 64), seed=90).to(DEV), make_input("audio", (2, 96, 64), seed=91).to(DEV),
            make_input("audio", (2, 128, 64), seed=92).to(DEV)]           # the third: other shapes than the graph's, an eager step
    tr = Trainer(d, dataloader=data, train_lr=1e-3, train_num_steps=4, ema_update_every=2, results_folder=tmp_path / "run",
                 save_and_sample_every=4, num_samples=1, sample_length=96)
    tr.train()
    assert tr.step == 4 and int(tr.opt.steps_taken) == 4
    at4 = _state(tr.opt, list(d.parameters()))
    tr.train_num_steps = 8
    tr.train()
    assert tr.step == 8 and int(tr.opt.steps_taken) == 8
    assert _same_bits({"p": at4["p"]}, {"p": [p.detach() for p in d.parameters()]}) is not None
    for name in ("model-1.pt", "model-2.pt", "sample_4.pt", "sample_4.ema.pt", "sample_8.pt", "sample_8.ema.pt"):
        assert (tmp_path / "run" / name).exists(), name
    assert torch.isfinite(torch.load(tmp_path / "run" / "sample_8.ema.pt")).all()

    m2, d2 = _model("exact", seed=6)
    fresh = Trainer(d2, dataloader=data, train_lr=1e-3, ema_update_every=2, results_folder=tmp_path / "run", sample_length=96)
    fresh.load(1)
    assert fresh.step == 4
    assert _same_bits(at4, _state(fresh.opt, list(d2.parameters()))) is None
    ck = torch.load(tmp_path / "run" / "model-1.pt", map_location="cpu")
    assert sorted(ck) == ["ema", "model", "opt", "scaler", "step", "version"]
    adam = torch.optim.Adam(d2.parameters())
    adam.load_state_dict(ck["opt"])
    p0 = next(iter(d2.parameters()))
    assert float(adam.state[p0]["step"]) == 4.0 and torch.equal(adam.state[p0]["exp_avg"].cpu(), at4["m"][0].cpu())
    em = fresh.ema_model
    assert all(torch.equal(a, b) for a, b in zip([p.detach() for p in em.parameters()], at4["ema"]))
    em.refresh_weights()
    out = em.sample(length=96, batch_size=1)
    assert out.shape == (1, 96, 64) and torch.isfinite(out).all()
    fresh.train_num_steps = 6                                              # ... and training goes on from the checkpoint
    fresh.train()
    assert int(fresh.opt.steps_taken) == 6


def test_trainer_accumulates_gradients_eagerly(tmp_path):
    m, d = _model("mixed", seed=7)
    data = [make_input("audio", (2, 96, 64), seed=93 + i).to(DEV) for i in range(2)]
    tr = Trainer(d, dataloader=data, train_lr=1e-3, train_num_steps=2, gradient_accumulate_every=2, use_ema=False,
                 save_and_sample_every=0, results_folder=tmp_path / "acc")
    p0 = [p.detach().clone() for p in d.parameters()]
    tr.train()
    assert tr._graph is None and int(tr.opt.steps_taken) == 2 and int(tr.opt.skipped) == 0
    assert torch.isfinite(tr.last_loss) and torch.isfinite(tr.opt.grad_norm)
    assert any(not torch.equal(a, p.detach()) for a, p in zip(p0, d.parameters()))
