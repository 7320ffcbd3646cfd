"""Checks of the fused SGD / LARS optimizers (ccd_amd.optim.FusedClipSGD / FusedClipLARS and the kernels under them), shared by
test_optim_cpu.py (no kernels), test_optim_sim.py (CPU SIMT executor) and test_optim_gpu.py (-m gpu).

The yardsticks are tests/golden/optim_cases.npz - the reference's clip_gradients -> cancel_gradients_last_layer -> torch.optim.SGD /
LARS recorded by tools/gen_optim_golden.py - and `step64`, a float64 restatement of the two update rules.

Gates (where they come from):
  restatement vs fixture   parameters and SGD buffers rtol 1e-6 / atol 1e-7 (fp32 rounding of one step); LARS mu rtol 2e-4 (the
                           reference's own fp32 torch.norm is ~5e-5 off fp64, and two norms enter q as a ratio)
  three-sum table          rtol 1e-4 against fp64 (the existing opt/norm2 gate); sum g p, which may be near zero, gets an atol of
                           1e-4 sqrt(sum g^2 sum p^2) (Cauchy-Schwarz: the size its terms have)
  update kernels           parameters rtol 1e-5 / atol 1e-6 (the existing opt/param gate), SGD buffers the same; LARS mu rtol 2e-4
                           (two norms, each good to half of the 1e-4 squared-norm gate, enter q as a ratio) with atol 1e-8 (one ulp
                           of the 0.1-sized old buffer it is summed with); mirror == bf16(parameter) bit for bit
"""
import json
import os

import numpy as np
import torch

KINDS = ("sgd", "lars")
STATE_KEY = {"sgd": "momentum_buffer", "lars": "mu"}
BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------ fixture + restatement
def load_cases(golden_dir):
    z = np.load(os.path.join(golden_dir, "optim_cases.npz"))
    c = {k: z[k] for k in z.files}
    c["names"] = [str(n) for n in c["names"]]
    c["never_used"] = [str(n) for n in c["never_used"]]
    c["layouts"] = json.loads(str(c["layouts"]))
    c["iters"] = len(c["lr"])
    return c


def step64(kind, p, buf, g, lr, wd, ndim, clip=3.0, momentum=0.9, eta=0.001):
    """One tensor, one iteration, in float64: per-tensor clip, then torch.optim.SGD(momentum) or the reference's LARS.
    g None = the tensor has no gradient this iteration: nothing changes.  -> (p, buf)"""
    p, buf = p.double(), buf.double()
    if g is None:
        return p, buf
    g = g.double()
    if clip > 0:
        coef = clip / (g.norm() + 1e-6)
        if coef < 1:
            g = g * coef
    if kind == "sgd":
        d = g + wd * p
    elif ndim != 1:
        d = g + wd * p
        pn, dn = p.norm(), d.norm()
        if pn > 0 and dn > 0:
            d = d * (eta * pn / dn)
    else:
        d = g
    buf = momentum * buf + d
    return p - lr * buf, buf


def close64(got, want, rtol, atol, what):
    got, want = got.detach().double().cpu().reshape(-1), want.detach().double().cpu().reshape(-1)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    err = (got - want).abs()
    bad = ~(err <= atol + rtol * want.abs())
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {err.max().item():.4g} "
                           f"(want max {want.abs().max().item():.4g})")


def fixture_gradient(c, it, i):
    """The gradient the optimizer sees for tensor i at iteration `it` (None: never used, or the cancelled last layer)."""
    name = c["names"][i]
    if f"g/{it}/{i}" not in c or ("last_layer" in name and c["epoch"][it] < c["freeze_last_layer"]):
        return None
    return torch.from_numpy(c[f"g/{it}/{i}"])


def group_wd(c, kind, name, it):
    return float(c["wd"][it]) if name in c["layouts"][kind]["group_names"][0] else 0.0


def check_restatement_matches_fixture(golden_dir):
    """step64 from the recorded fp32 state of iteration it-1 reproduces the recorded state of iteration it, every tensor."""
    c = load_cases(golden_dir)
    for kind in KINDS:
        for i, name in enumerate(c["names"]):
            p, buf = torch.from_numpy(c[f"p0/{i}"]), torch.zeros(c[f"p0/{i}"].shape)
            for it in range(c["iters"]):
                g = fixture_gradient(c, it, i)
                p64, b64 = step64(kind, p, buf, g, float(c["lr"][it]), group_wd(c, kind, name, it), p.dim(),
                                  float(c["clip"]), float(c["momentum"]), float(c["eta"]))
                p, buf = torch.from_numpy(c[f"{kind}/p/{it}/{i}"]), torch.from_numpy(c[f"{kind}/buf/{it}/{i}"])
                what = f"{kind}/{name}/it{it}"
                close64(p, p64, 1e-6, 1e-7, what + "/param")
                close64(buf, b64, 2e-4 if kind == "lars" else 1e-6, 1e-7, what + "/buf")
                if g is None and not bool(c[f"{kind}/has_state/{it}/{i}"]):
                    assert not buf.any(), what


# ------------------------------------------------------------------------------------------------ small arenas
class HostArena:
    """The host-side bookkeeping of ccd_amd.arena.ParamArena (segments, parameters, one flat fp32 buffer) without its device
    mirrors: enough for the optimizers' constructor, stage_hyper and checkpoint code, none of which launches a kernel."""

    def __init__(self, named_params):
        from ccd_amd.arena import ALIGN, Segment
        self.device = torch.device("cpu")
        self.segments, self.params, off = {}, {}, 0
        for i, (name, p) in enumerate(named_params):
            self.segments[name] = Segment(name, off, p.numel(), p.shape, i)
            self.params[name] = p
            off += (p.numel() + ALIGN - 1) // ALIGN * ALIGN
        self.flat = torch.zeros(off)
        self.skip_substrings = set()


def fixture_params(c):
    return [(n, torch.nn.Parameter(torch.from_numpy(c[f"p0/{i}"]).clone())) for i, n in enumerate(c["names"])]


def make(kind, arena, **kw):
    from ccd_amd import optim
    return {"adamw": optim.FusedClipAdamW, "sgd": optim.FusedClipSGD, "lars": optim.FusedClipLARS}[kind](arena, **kw)


def check_checkpoint_layouts(golden_dir):
    """SGD: torch.optim.SGD's layout (loads into a real one built on the same groups, and round-trips); LARS: the reference
    class's recorded key sets; a tensor that never stepped has no entry; cross-kind loads raise ValueError naming both kinds."""
    c = load_cases(golden_dir)
    opts = {}
    for kind in ("adamw",) + KINDS:
        opt = make(kind, HostArena(fixture_params(c)), clip_grad=3.0)
        opt.mark_unused(c["never_used"])
        gen = torch.Generator().manual_seed(5)
        for t in ([opt.exp_avg, opt.exp_avg_sq] if kind == "adamw" else [opt.buf]):
            t.copy_(torch.randn(t.shape, generator=gen))
        opt.arena.skip_substrings.add("last_layer")
        for gi, g in enumerate(opt.param_groups):
            g["lr"], g["weight_decay"] = 0.125, (0.25 if gi == 0 else 0.0)
        opt.stage_hyper()                                    # one step's host half: every active tensor now has state
        opts[kind] = opt
    for kind in KINDS:
        opt, lay = opts[kind], c["layouts"][kind]
        sd = opt.state_dict()
        assert [g["names"] for g in opt.param_groups] == lay["group_names"]
        assert [sorted(g) for g in sd["param_groups"]] == lay["group_keys"], (kind, [sorted(g) for g in sd["param_groups"]])
        assert [g["params"] for g in sd["param_groups"]] == lay["group_params"]
        assert {k for st in sd["state"].values() for k in st} == set(lay["state_keys"]) == {STATE_KEY[kind]}
        flat_names = [n for g in opt.param_groups for n in g["names"]]
        silent = {i for i, n in enumerate(flat_names) if n in c["never_used"] or "last_layer" in n}
        assert set(sd["state"]) == set(range(len(flat_names))) - silent
        for i, st in sd["state"].items():
            seg = opt.arena.segments[flat_names[i]]
            assert st[STATE_KEY[kind]].shape == seg.shape
            assert torch.equal(st[STATE_KEY[kind]].reshape(-1), opt.buf[seg.offset:seg.offset + seg.numel])
        assert sd["param_groups"][0]["lr"] == 0.125 and sd["param_groups"][0]["weight_decay"] == 0.25
        assert sd["param_groups"][1]["weight_decay"] == 0.0 and sd["param_groups"][0]["momentum"] == 0.9
        if kind == "lars":
            assert sd["param_groups"][0]["eta"] == 0.001
        # round trip through torch.save / a fresh optimizer
        fresh = make(kind, HostArena(fixture_params(c)), clip_grad=3.0)
        fresh.load_state_dict(sd)
        assert torch.equal(fresh.buf, torch.where(_stepped_mask(opt), opt.buf, torch.zeros(())))
        assert fresh.stepped == opt.stepped and fresh.param_groups[0]["lr"] == 0.125
        sd2 = fresh.state_dict()
        assert set(sd2["state"]) == set(sd["state"]) and sd2["param_groups"] == sd["param_groups"]
        # every other kind's state is refused, by name
        for other in ("adamw",) + KINDS:
            if other == kind:
                continue
            try:
                make(kind, HostArena(fixture_params(c))).load_state_dict(opts[other].state_dict())
            except ValueError as e:
                assert f"'{other}'" in str(e) and f"'{kind}'" in str(e), str(e)
            else:
                raise AssertionError(f"{kind} loaded a {other} state")
    for other in KINDS:                                      # and AdamW refuses theirs the same way
        try:
            make("adamw", HostArena(fixture_params(c))).load_state_dict(opts[other].state_dict())
        except ValueError as e:
            assert f"'{other}'" in str(e) and "'adamw'" in str(e), str(e)
        else:
            raise AssertionError(f"adamw loaded a {other} state")
    # the SGD dict is torch.optim.SGD's: a real one on the same groups takes it and gives it back
    opt = opts["sgd"]
    sd = opt.state_dict()
    real = torch.optim.SGD([{"params": opt.param_groups[0]["params"]}, {"params": opt.param_groups[1]["params"], "weight_decay": 0.0}],
                           lr=0.0, momentum=0.9)
    real.load_state_dict(sd)
    back = real.state_dict()
    assert back["param_groups"] == sd["param_groups"]
    assert set(back["state"]) == set(sd["state"])
    for i in sd["state"]:
        assert set(back["state"][i]) == {"momentum_buffer"}
        assert torch.equal(back["state"][i]["momentum_buffer"], sd["state"][i]["momentum_buffer"])
    again = make("sgd", HostArena(fixture_params(c)))
    again.load_state_dict(back)
    assert torch.equal(again.buf, torch.where(_stepped_mask(opt), opt.buf, torch.zeros(())))


def _stepped_mask(opt):
    m = torch.zeros(opt.buf.shape, dtype=torch.bool)
    for n in opt.stepped:
        seg = opt.arena.segments[n]
        m[seg.offset:seg.offset + seg.numel] = True
    return m


# ------------------------------------------------------------------------------------------------ kernels (sim and GPU)
def check_moment_kernels(dev, seed=13):
    """ccd_seg_moments / ccd_sgd_momentum / ccd_lars on odd sizes with an inactive tensor: the twin of kernel_checks.check_optimizer."""
    from ccd_amd import ops
    from kernel_checks import close, rnd
    gen = torch.Generator().manual_seed(seed)
    sizes = [5, 1024, 1500, 64, 3000]
    dims = [2, 1, 2, 2, 3]                                  # LARS adapts by ndim: tensor 1 is 1-D
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + 63) // 64 * 64
    param = rnd((total,), gen); grad = rnd((total,), gen) * torch.tensor(3.0)
    grad[offs[2]:offs[2] + sizes[2]] *= 0.001          # a tensor whose norm stays under the clip
    chunk_seg, chunk_begin, chunk_len = [], [], []
    for s_, (o, n) in enumerate(zip(offs, sizes)):
        for c in range(0, n, 1024):
            chunk_seg.append(s_); chunk_begin.append(o + c); chunk_len.append(min(1024, n - c))
    cs = torch.tensor(chunk_seg, dtype=torch.int32).to(dev)
    cb = torch.tensor(chunk_begin, dtype=torch.int64).to(dev)
    cl = torch.tensor(chunk_len, dtype=torch.int32).to(dev)
    lr, wd, clip, mom, eta = 3e-2, 0.1, 3.0, 0.9, 0.001
    active = [1, 1, 1, 0, 1]
    decay = [1, 0, 1, 1, 1]
    hyper = torch.tensor([[lr, wd * d, float(nd != 1), a] for d, a, nd in zip(decay, active, dims)], dtype=torch.float32).to(dev)
    buf0 = rnd((total,), gen) * 0.1
    for kind in KINDS:
        p0 = param.clone()
        if kind == "lars":
            p0[offs[0]:offs[0] + sizes[0]] = 0.0            # |p| = 0: the trust ratio is 1
        G, Pd, Bd = grad.to(dev), p0.clone().to(dev), buf0.clone().to(dev)
        mirror = torch.full((total,), 7.0, dtype=BF).to(dev)
        if kind == "sgd":
            norm2 = torch.zeros(len(sizes)).to(dev)
            ops.seg_sumsq(G, cs, cb, cl, norm2)
            ops.sgd_momentum(Pd, G, Bd, mirror, cs, cb, cl, hyper, norm2, clip, mom)
        else:
            moments = torch.zeros(len(sizes), 3).to(dev)
            ops.seg_moments(G, Pd, cs, cb, cl, moments)
            g64, p64 = grad.double(), p0.double()
            want = torch.stack([torch.stack([g64[o:o + n].pow(2).sum(), p64[o:o + n].pow(2).sum(), (g64[o:o + n] * p64[o:o + n]).sum()])
                                for o, n in zip(offs, sizes)])
            got = moments.double().cpu()
            close64(got[:, 0], want[:, 0], 1e-4, 0.0, "lars/sum g^2")
            close64(got[:, 1], want[:, 1], 1e-4, 0.0, "lars/sum p^2")
            cross_err = (got[:, 2] - want[:, 2]).abs()
            cross_tol = 1e-4 * want[:, 2].abs() + 1e-4 * (want[:, 0] * want[:, 1]).sqrt()
            assert bool((cross_err <= cross_tol).all()), ("lars/sum g p", cross_err, cross_tol)
            ops.lars(Pd, G, Bd, mirror, cs, cb, cl, hyper, moments, clip, mom, eta)
        for s_, (o, n) in enumerate(zip(offs, sizes)):
            sl = slice(o, o + n)
            if not active[s_]:                               # bit-unchanged: parameter, buffer and mirror
                assert torch.equal(Pd[sl].cpu(), p0[sl]) and torch.equal(Bd[sl].cpu(), buf0[sl]), f"{kind}/inactive{s_}"
                assert bool((mirror[sl].float().cpu() == 7.0).all()), f"{kind}/inactive-mirror{s_}"
                continue
            p, b = step64(kind, p0[sl], buf0[sl], grad[sl], lr, wd * decay[s_], dims[s_], clip, mom, eta)
            close(Pd[sl], p, 1e-5, 1e-6, f"{kind}/param{s_}")
            if kind == "sgd":
                close(Bd[sl], b, 1e-5, 1e-6, f"{kind}/buf{s_}")
            else:
                close64(Bd[sl], b, 2e-4, 1e-8, f"{kind}/mu{s_}")
            assert torch.equal(mirror[sl].cpu(), Pd[sl].cpu().to(BF)), f"{kind}/mirror{s_}"
            close(mirror[sl], p.float().to(BF), 1e-2, 1e-6, f"{kind}/mirror-vs-restatement{s_}")
        # nothing behind a tensor's last element was written (the alignment gaps of the arena)
        for o, n in zip(offs, sizes):
            gap = slice(o + n, o + (n + 63) // 64 * 64)
            assert torch.equal(Pd[gap].cpu(), p0[gap]) and torch.equal(Bd[gap].cpu(), buf0[gap]), f"{kind}/gap"
    # clip off: the coefficient is 1 whatever the norm table holds
    G, Pd, Bd = grad.to(dev), param.clone().to(dev), buf0.clone().to(dev)
    ops.sgd_momentum(Pd, G, Bd, None, cs, cb, cl, hyper, torch.full((len(sizes),), 1e6).to(dev), 0.0, mom)
    o, n = offs[1], sizes[1]
    p, b = step64("sgd", param[o:o + n], buf0[o:o + n], grad[o:o + n], lr, 0.0, 1, 0.0, mom)
    close(Pd[o:o + n], p, 1e-5, 1e-6, "sgd/no-clip param")
    close(Bd[o:o + n], b, 1e-5, 1e-6, "sgd/no-clip buf")


def check_fixture_replay(dev, golden_dir):
    """The fixture's iterations through FusedClipSGD / FusedClipLARS on a real ParamArena of the fixture's tensors, at the kernel
    gates: lr / wd of each iteration, the last layer cancelled on the first two, a never-used tensor, an all-zero parameter."""
    from ccd_amd.arena import ParamArena
    c = load_cases(golden_dir)
    for kind in KINDS:
        params = fixture_params(c)
        arena = ParamArena(params, dev)
        opt = make(kind, arena, clip_grad=float(c["clip"]))
        opt.mark_unused(c["never_used"])
        assert [g["names"] for g in opt.param_groups] == c["layouts"][kind]["group_names"]
        for it in range(c["iters"]):
            for gi, g in enumerate(opt.param_groups):
                g["lr"] = float(c["lr"][it])
                if gi == 0:
                    g["weight_decay"] = float(c["wd"][it])
            opt.zero_grad()
            for i, n in enumerate(c["names"]):
                if f"g/{it}/{i}" in c:
                    arena.g(n).copy_(torch.from_numpy(c[f"g/{it}/{i}"]))
            if c["epoch"][it] < c["freeze_last_layer"]:
                arena.skip_substrings.add("last_layer")
            opt.step()
            sd = opt.state_dict()
            flat_names = [n for g in opt.param_groups for n in g["names"]]
            for i, n in enumerate(c["names"]):
                what = f"{kind}/{n}/it{it}"
                seg = arena.segments[n]
                buf = opt.buf[seg.offset:seg.offset + seg.numel]
                want_p, want_b = torch.from_numpy(c[f"{kind}/p/{it}/{i}"]), torch.from_numpy(c[f"{kind}/buf/{it}/{i}"])
                close64(arena.w(n), want_p, 1e-5, 1e-6, what + "/param")
                close64(buf, want_b, 2e-4 if kind == "lars" else 1e-5, 1e-8 if kind == "lars" else 1e-6, what + "/buf")
                assert torch.equal(arena.wb(n).cpu(), arena.w(n).cpu().to(BF)), what + "/mirror"
                assert (flat_names.index(n) in sd["state"]) == bool(c[f"{kind}/has_state/{it}/{i}"]), what + "/state entry"
                if not bool(c[f"{kind}/has_state/{it}/{i}"]):
                    assert torch.equal(arena.w(n).cpu(), torch.from_numpy(c[f"p0/{i}"])) and not buf.any(), what + "/untouched"


# ------------------------------------------------------------------------------------------------ model level (sim and GPU)
LR_SCALE = {"sgd": 10.0, "lars": 20.0}      # x the AdamW checks' 1e-3: a clipped SGD step moves lr * 3 per tensor at most, a LARS
                                            # step lr * 1e-3 |p| - kept well above the fp32 rounding of the parameters


def check_host_runs_ahead(device, kind, steps=8):
    """model_checks.check_optimizer_host_runs_ahead for the new classes: the host refills the per-tensor table for step N+1 while
    the copy of step N may not have executed; every step must still see ITS lr / weight decay."""
    import model_checks as mc
    from ccd_amd import pretrain
    results = []
    for sync_each in (True, False):
        student, _ = mc.tiny_networks(device)
        opt = pretrain.make_optimizer(student, clip_grad=3.0, name=kind)
        assert type(opt).__name__ == {"sgd": "FusedClipSGD", "lars": "FusedClipLARS"}[kind]
        g = torch.Generator().manual_seed(0)
        grads = [torch.randn(student.arena.grad.shape, generator=g).to(device) for _ in range(steps)]
        if not sync_each and device.type == "cuda":        # back the stream up so that the host really runs ahead
            a = torch.randn(4096, 4096, device=device)
            for _ in range(40):
                a = (a @ a) * 1e-4
        for i in range(steps):
            for gi, grp in enumerate(opt.param_groups):
                grp["lr"] = 1e-3 * LR_SCALE[kind] * (1 + 7 * (i % 3))          # very different from step to step
                if gi == 0:
                    grp["weight_decay"] = 0.05 * (1 + i)
            student.arena.grad.copy_(grads[i])
            opt.step()
            if sync_each and device.type == "cuda":
                torch.cuda.synchronize()
        if device.type == "cuda":
            torch.cuda.synchronize()
        results.append((student.arena.flat.clone(), opt.buf.clone(), student.arena.mirror.clone()))
    start = mc.tiny_networks(device)[0].arena.flat
    diff = (results[0][0] - results[1][0]).abs().max().item()
    move = (results[0][0] - start).abs().max().item()
    assert move > 0 and diff <= 1e-4 * move, f"{kind}: steps saw another step's hyper-parameters (diff {diff}, update {move})"
    bdiff = (results[0][1] - results[1][1]).abs().max().item()
    assert bdiff <= 1e-4 * results[0][1].abs().max().item(), (kind, bdiff)
    assert torch.equal(results[1][2], results[1][0].to(BF)), f"{kind}: bf16 mirror is stale"
    # never-used tensors did not move, and hold no state
    student, _ = mc.tiny_networks(device)
    arena = student.arena
    for n in student.unused_parameter_names():
        seg = arena.segments[n]
        sl = slice(seg.offset, seg.offset + seg.numel)
        assert torch.equal(results[1][0][sl], start[sl]) and not results[1][1][sl].any(), n


def check_checkpoint_resume(device, tmp_path, kind):
    """model_checks.check_checkpoint_resume with `optimizer: sgd / lars`: the reference's checkpoint layout restored into freshly
    built networks - state bit-identical, the next iteration's loss reproduced; an AdamW run over the same file starts fresh."""
    import model_checks as mc
    from ccd_amd import pretrain
    from ccd_amd.loss.Dino_loss import DINOLoss
    from ccd_amd.modules import utils
    from ccd_amd.parallel import DataParallel
    from ccd_amd.synthetic import make_batch
    lr = 2e-4 * LR_SCALE[kind]

    def build(name=kind):
        student, teacher = mc.tiny_networks(device)
        s, t = DataParallel(student), DataParallel(teacher)
        t.module.backbone.load_state_dict(s.module.backbone.state_dict())
        t.module.head.load_state_dict(s.module.head.state_dict())
        t.module.ensure_arena()
        loss = DINOLoss(512, 2, 0.04, 0.04, 0, 40).to(device)
        return s, t, loss, pretrain.make_optimizer(s.module, clip_grad=3.0, name=name)

    def run(s, t, loss, opt, seed, epoch):
        images, masks, metrics = make_batch(1, seed=seed, device=device)
        return float(pretrain.training_iteration(s, t, loss, opt, images, masks, metrics, epoch, lr, 0.05, 0.99).item())

    s, t, loss, opt = build()
    run(s, t, loss, opt, seed=20, epoch=0)                     # last layer frozen: it must come back WITHOUT state
    run(s, t, loss, opt, seed=21, epoch=0)
    path = os.path.join(str(tmp_path), f"checkpoint_{kind}.pth")
    torch.save({"student": s.state_dict(), "teacher": t.state_dict(), "optimizer": opt.state_dict(), "epoch": 1,
                "iteration": 2, "dino_loss": loss.state_dict()}, path)
    saved = torch.load(path, map_location="cpu", weights_only=False)["optimizer"]
    assert {k for st in saved["state"].values() for k in st} == {STATE_KEY[kind]}
    flat_names = [n for g in opt.param_groups for n in g["names"]]
    silent = {i for i, n in enumerate(flat_names) if "last_layer" in n or n in opt.never_used}
    assert silent and set(saved["state"]) == set(range(len(flat_names))) - silent
    snap = {"flat": s.module.arena.flat.clone(), "tflat": t.module.arena.flat.clone(), "buf": opt.buf.clone(),
            "stepped": set(opt.stepped), "center": loss.center.clone()}
    assert snap["buf"].any()
    want = run(s, t, loss, opt, seed=22, epoch=1)

    torch.manual_seed(99)                                      # different initial weights: everything must come from the file
    s2, t2, loss2, opt2 = build()
    restored = {"epoch": 0, "iteration": 0}
    utils.restart_from_checkpoint(path, run_variables=restored, student=s2, teacher=t2, optimizer=opt2, dino_loss=loss2)
    assert restored == {"epoch": 1, "iteration": 2}
    s2.module.ensure_arena()
    t2.module.ensure_arena()
    assert torch.equal(s2.module.arena.flat, snap["flat"]) and torch.equal(t2.module.arena.flat, snap["tflat"])
    assert torch.equal(opt2.buf, snap["buf"]) and opt2.stepped == snap["stepped"]
    assert torch.equal(loss2.center, snap["center"])
    got = run(s2, t2, loss2, opt2, seed=22, epoch=1)
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (got, want)
    # the YAML switched back to adamw over this checkpoint directory: the weights load, the optimizer starts fresh (and says so)
    s3, t3, loss3, opt3 = build("adamw")
    utils.restart_from_checkpoint(path, run_variables={}, student=s3, teacher=t3, optimizer=opt3, dino_loss=loss3)
    assert not opt3.exp_avg.any() and not opt3.exp_avg_sq.any() and not any(opt3.steps.values())
    assert torch.equal(s3.module.arena.flat, snap["flat"])


def check_graphed_step_matches_eager(device, kind, steps=8, B=8, drop_path_rate=0.1):
    """model_checks.check_graphed_step_matches_eager with `optimizer: sgd / lars`: the iteration replayed as ONE HIP graph against
    the eager iteration, lr / weight decay / EMA momentum changing every iteration and the last layer frozen during epoch 0 - all
    of it reaches the captured update kernel through the staged table.  Same tolerances as the AdamW check."""
    import model_checks as mc
    from ccd_amd import engine, pretrain
    from ccd_amd.loss.Dino_loss import DINOLoss
    from ccd_amd.synthetic import make_batch
    out = []
    for graphed in (False, True):
        torch.manual_seed(3)
        np.random.seed(3)
        engine._DROPPATH_SEED.update(base=1234567, calls=0)
        student, teacher = pretrain.build_networks(arch=None, out_dim=512, drop_path_rate=drop_path_rate,
                                                   norm_last_layer=False, seg_channel=192,
                                                   backbone_kwargs=dict(embed_dim=192, depth=3, num_heads=3, out_indices=[1, 2, 3]),
                                                   head_kwargs=dict(hidden_dim=256, bottleneck_dim=64), device=device)
        dino_loss = DINOLoss(512, 2, 0.04, 0.07, 3, 40).to(device)
        opt = pretrain.make_optimizer(student, clip_grad=3.0, name=kind)
        run = pretrain.GraphedTrainingStep(student, teacher, dino_loss, opt, eager_steps=1) if graphed else None
        losses = []
        for i in range(steps):
            images, masks, metrics = make_batch(B, seed=50 + i, device=device)
            epoch = i // 2                                   # 0, 0, 1, 1, 2, 2, 3, 3: frozen last layer, three temperatures
            kw = dict(epoch=epoch, lr=1e-3 * LR_SCALE[kind] * (1 + i % 3), wd=0.04 * (1 + i), momentum=0.99 - 0.01 * i)
            if graphed:
                losses.append(run(images, masks, metrics, **kw))
            else:
                losses.append(pretrain.training_iteration(student, teacher, dino_loss, opt, images, masks, metrics, **kw))
        if device.type == "cuda":
            torch.cuda.synchronize()
        out.append(([float(l) for l in losses], student.arena.flat.clone(), teacher.arena.flat.clone(), dino_loss.center.clone(),
                    opt.buf.clone(), None if run is None else (run.captures, run.replays)))
    (le, se, te, ce, be, _), (lg, sg, tg, cg, bg, counts) = out
    temps = [float(DINOLoss(512, 2, 0.04, 0.07, 3, 40).teacher_temp_schedule[i // 2]) for i in range(1, steps)]
    want = 1 + sum(a_ != b_ for a_, b_ in zip(temps, temps[1:]))          # one capture per teacher temperature met
    assert counts == (want, steps - 1), (counts, want)
    assert all(np.isfinite(le)) and all(np.isfinite(lg)), (le, lg)
    for i, (a_, b_) in enumerate(zip(le, lg)):
        assert abs(a_ - b_) <= 1e-3 * max(1.0, abs(a_)), f"{kind} iteration {i}: eager loss {a_} vs graphed {b_}"
    s0, t0 = (n.arena.flat for n in mc.tiny_networks(device))
    move, t_move = (se - s0).norm().item(), (te - t0).norm().item()
    assert move > 0 and (se - sg).norm().item() <= 0.15 * move, (kind, (se - sg).norm().item(), move)
    assert (te - tg).norm().item() <= 0.15 * t_move, (kind, (te - tg).norm().item(), t_move)
    assert (ce - cg).norm().item() <= 0.05 * ce.norm().item(), (kind, (ce - cg).norm().item(), ce.norm().item())
    assert (be - bg).norm().item() <= 0.15 * be.norm().item(), (kind, (be - bg).norm().item(), be.norm().item())
