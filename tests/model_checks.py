"""End-to-end checks of the product stack (modules + engine + optimizer) against golden fixtures produced by the
real reference; run under the CPU SIMT executor (tiny model) and on the GPU."""
import os

import numpy as np
import torch

from ccd_amd import pretrain
from ccd_amd.loss.Dino_loss import DINOLoss
from ccd_amd.synthetic import make_batch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Every image contributes ONE all-zero pooled row per view (`grid <= length` keeps length+1 rows, dino_vision.py:82-85).
# While the head biases are still 0 such a row reaches F.normalize as an exact zero vector, whose backward multiplies by
# 1/eps = 1e12; the reference's incoming gradient there is fp32 rounding residue of (1/K - 1/K), so its head-bias
# gradients at that point are amplified noise (L2 ~ 1e2..1e4, then clipped to 3).  Ours are exactly 0 for those rows.
# Those three tensors are therefore excluded from gradient / post-step parity (documented in DESIGN.md).
NOISE_DOMINATED = ("head.mlp.0.bias", "head.mlp.2.bias", "head.mlp.4.bias")


def assert_init_stat(got, row, name):
    """[sum, abs-sum, l2] computed in fp64; only the summation ORDER may differ between hosts (thread counts)."""
    assert abs(got[0] - row[0]) <= 1e-9 * row[1] + 1e-12, f"init:{name} sum {got[0]} vs {row[0]}"
    np.testing.assert_allclose(got[1:], row[1:], rtol=1e-9, atol=1e-12, err_msg=f"init:{name}")


def stat(t):
    t = t.detach().double().cpu()
    return np.array([t.sum().item(), t.abs().sum().item(), t.pow(2).sum().sqrt().item()])


def tiny_networks(device):
    torch.manual_seed(3)
    np.random.seed(3)
    return pretrain.build_networks(arch=None, out_dim=512, drop_path_rate=0.0, norm_last_layer=False, seg_channel=192,
                                   backbone_kwargs=dict(embed_dim=192, depth=3, num_heads=3, out_indices=[1, 2, 3]),
                                   head_kwargs=dict(hidden_dim=256, bottleneck_dim=64), device=device)


def check_optimizer_host_runs_ahead(device, steps=8):
    """The host refills the per-tensor hyper-parameter table for step N+1 while the copy of step N may not have executed
    (train.py reads the loss one iteration late): every step must still see ITS lr / weight decay / bias correction.
    Reference: the same steps with a device synchronisation after each."""
    results = []
    for sync_each in (True, False):
        student, _ = tiny_networks(device)
        opt = pretrain.make_optimizer(student, clip_grad=3.0)
        g = torch.Generator().manual_seed(0)
        grads = [torch.randn(student.arena.grad.shape, generator=g).to(device) for _ in range(steps)]
        if not sync_each and device.type == "cuda":        # back the stream up so that the host really runs ahead
            a = torch.randn(4096, 4096, device=device)
            for _ in range(40):
                a = (a @ a) * 1e-4
        for i in range(steps):
            for gi, grp in enumerate(opt.param_groups):
                grp["lr"] = 1e-3 * (1 + 7 * (i % 3))          # very different from step to step
                if gi == 0:
                    grp["weight_decay"] = 0.05 * (1 + i)
            student.arena.grad.copy_(grads[i])
            opt.step()
            if sync_each and device.type == "cuda":
                torch.cuda.synchronize()
        if device.type == "cuda":
            torch.cuda.synchronize()
        results.append(student.arena.flat.clone())
    # (not bit-equal: the per-tensor gradient norms are sums of fp32 atomics; a wrong lr is a 2x .. 8x error in the update)
    diff = (results[0] - results[1]).abs().max().item()
    move = (results[0] - tiny_networks(device)[0].arena.flat).abs().max().item()
    assert diff <= 1e-4 * move, f"optimizer steps saw another step's hyper-parameters (diff {diff}, update {move})"


def check_graphed_step_matches_eager(device, steps=8, B=8, drop_path_rate=0.1):
    """pretrain.GraphedTrainingStep (the iteration replayed as ONE HIP graph) against the eager iteration on the same batches
    and schedules: lr / weight decay / momentum change every iteration, the last layer is frozen during pseudo-epoch 0
    (train.py:247-248), the teacher temperature warms up over 3 epochs (=> re-captures) and DropPath is on (the graph's
    device-side seed must follow the eager seed sequence).  Not bit-equal (fp32 atomics in the weight-gradient epilogues)."""
    from ccd_amd import engine
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
        opt = pretrain.make_optimizer(student, clip_grad=3.0)
        run = pretrain.GraphedTrainingStep(student, teacher, dino_loss, opt, eager_steps=1) if graphed else None
        losses = []
        for i in range(steps):
            images, masks, metrics = make_batch(B, seed=50 + i, device=device)
            epoch = i // 2                                   # 0, 0, 1, 1, 2, 2, 3, 3: frozen last layer, three temperatures
            kw = dict(epoch=epoch, lr=1e-3 * (1 + i % 3), wd=0.04 * (1 + i), momentum=0.99 - 0.01 * i)
            if graphed:
                losses.append(run(images, masks, metrics, **kw))
            else:
                losses.append(pretrain.training_iteration(student, teacher, dino_loss, opt, images, masks, metrics, **kw))
        if device.type == "cuda":
            torch.cuda.synchronize()
        out.append(([float(l) for l in losses], student.arena.flat.clone(), teacher.arena.flat.clone(), dino_loss.center.clone(),
                    None if run is None else (run.captures, run.replays)))
    (le, se, te, ce, _), (lg, sg, tg, cg, counts) = out
    temps = [float(DINOLoss(512, 2, 0.04, 0.07, 3, 40).teacher_temp_schedule[i // 2]) for i in range(1, steps)]
    want = 1 + sum(a_ != b_ for a_, b_ in zip(temps, temps[1:]))          # one capture per teacher temperature met
    assert counts == (want, steps - 1), (counts, want)
    for i, (a_, b_) in enumerate(zip(le, lg)):
        assert abs(a_ - b_) <= 1e-3 * max(1.0, abs(a_)), f"iteration {i}: eager loss {a_} vs graphed {b_}"
    # updates compared in L2: an Adam step on a small batch turns atomics-order noise into +- lr element-wise - two EAGER runs
    # of this schedule differ by ~5 % of the distance moved (measured on the CPU executor); a step that saw another
    # iteration's lr / momentum / masks is an O(1) error
    s0, t0 = (n.arena.flat for n in tiny_networks(device))
    move, t_move = (se - s0).norm().item(), (te - t0).norm().item()
    assert (se - sg).norm().item() <= 0.15 * move, ((se - sg).norm().item(), move)
    assert (te - tg).norm().item() <= 0.15 * t_move, ((te - tg).norm().item(), t_move)
    assert (ce - cg).norm().item() <= 0.05 * ce.norm().item(), ((ce - cg).norm().item(), ce.norm().item())


def check_tiny_step(device, logit_tol=3e-2, loss_tol=None, grad_rtol=6e-2, batch=2):
    """The reference's 3-block E = 192 model, every stage + one full iteration.  batch = 8 (tiny8_step.npz) is the GPU gate at the
    north-star tolerance 1e-3; batch = 2 (tiny_step.npz, what the CPU executor can afford) averages ~14 selected rows in its loss,
    whose bf16 logit noise does not average out - measured over seeds in profiles/r04_parity_tiny_budget.json - and keeps 2e-3."""
    if loss_tol is None:
        loss_tol = 1e-3 if batch >= 8 else 2e-3
    g = np.load(os.path.join(GOLD, "tiny_step.npz" if batch == 2 else f"tiny{batch}_step.npz"))
    student, teacher = tiny_networks(device)
    # 1. same seed -> bit-identical initial weights as the reference (construction order / RNG stream)
    sd = student.state_dict()
    for n, row in zip(g["init_names"], g["init_stats"]):
        assert_init_stat(stat(sd[str(n)]), row, n)
    dino_loss = DINOLoss(512, 2, 0.04, 0.04, 0, 40).to(device)
    opt = pretrain.make_optimizer(student, clip_grad=float(g["hyper"][4]))
    images, masks, metrics = make_batch(batch, seed=11, device=device)
    epoch, lr, wd, mom, clip, freeze = g["hyper"]
    # forward pieces first (so individual stages can be compared), then the full iteration on fresh grads
    bn_state = {k: v.clone() for k, v in student.state_dict().items() if "running_" in k or "num_batches" in k}
    s_out = student(images, metrics, masks, int(epoch))
    sel = s_out.raw("selection")
    np.testing.assert_array_equal(sel.idmap.cpu().numpy(), g["zero_idmap"])                # bit-exact index map
    np.testing.assert_array_equal(s_out["index"].cpu().numpy(), g["new_index"])
    M = sel.M
    assert 2 * M == g["student_logits"].shape[0]
    err = (s_out["mask"].detach().float().cpu().numpy() - g["seg_logits"])
    assert np.abs(err).max() < 5e-2 * max(1.0, np.abs(g["seg_logits"]).max()), f"seg logits off by {np.abs(err).max()}"
    got = s_out["instances_view"].detach().float().cpu().numpy()
    assert np.abs(got - g["student_logits"]).max() < logit_tol, np.abs(got - g["student_logits"]).max()
    with torch.no_grad():
        t_out = teacher(images, metrics, None, None, clusters=s_out["zero"])
    got_t = t_out["instances_view"].float().cpu().numpy()
    assert np.abs(got_t - g["teacher_logits"]).max() < logit_tol
    feat = t_out["feature"].float().cpu().numpy()[:, ::4]
    assert np.abs(feat - g["teacher_feature"]).max() < 6e-2, np.abs(feat - g["teacher_feature"]).max()
    del s_out, t_out
    student.load_state_dict(bn_state, strict=False)     # the stage-by-stage forward above must not count as a BN step
    loss = pretrain.training_iteration(student, teacher, dino_loss, opt, images, masks, metrics, int(epoch), lr, wd, mom,
                                       freeze_last_layer=int(freeze))
    losses = np.array([loss.item(), dino_loss.last_losses["mask_loss"].item(), dino_loss.last_losses["Dino_loss"].item()])
    np.testing.assert_allclose(losses, g["losses"], atol=loss_tol, rtol=0)
    np.testing.assert_allclose(dino_loss.center.cpu().numpy(), g["center_after"], rtol=0, atol=2e-3)
    # gradients (pre-clip) against the reference's autograd: L2 norms of every tensor + a few full tensors
    arena = student.arena
    worst = 0.0
    for n, row in zip(g["grad_names"], g["grad_stats"]):
        got_l2 = arena.g(str(n)).double().pow(2).sum().sqrt().item()
        if str(n) in NOISE_DOMINATED:
            continue
        if row[2] > 1e-6:
            worst = max(worst, abs(got_l2 - row[2]) / row[2])
            assert abs(got_l2 - row[2]) <= grad_rtol * row[2] + 1e-7, f"grad norm {n}: {got_l2} vs {row[2]}"
    for k in g.files:
        if k.startswith("grad/"):
            want = g[k]
            got_g = arena.g(k[5:]).float().cpu().numpy().reshape(want.shape)
            # elementwise: the segmentation branch's gradients are 1e-4 .. 1e-3 in size (three orders below the backbone's) and carry
            # 10 - 12 % of bf16 noise in rms at any batch (tools/lab/tiny_grad_err.py: norm_seg.1.weight 0.112 / 0.125 rms, 0.154 / 0.105
            # max at 8 / 2 images; everything in the backbone and the head < 0.015) - bounded in rms and, looser, in the maximum
            denom = np.abs(want).max() + 1e-12
            rms = np.sqrt(np.mean((got_g - want) ** 2)) / (np.sqrt(np.mean(want ** 2)) + 1e-12)
            assert rms < 0.15, f"{k}: rms rel err {rms}"
            seg_branch = k[5:].startswith(("segmentation.", "backbone.norm_seg."))      # (only these carry the looser maximum)
            assert np.abs(got_g - want).max() / denom < (0.2 if seg_branch else 0.15), f"{k}: rel err {np.abs(got_g - want).max() / denom}"
    # post-step weights and teacher EMA
    sd = student.state_dict()
    for n, row in zip(g["post_names"], g["post_stats"]):
        got_s = stat(sd[str(n)])
        if "num_batches_tracked" in str(n) or str(n) in NOISE_DOMINATED:
            continue
        # Adam's first steps move EVERY element by ~lr, also where the true gradient is exactly 0 and only rounding
        # noise decides the sign (e.g. the key bias of qkv, to which softmax is invariant): bound by the step size
        slack = 2.0 * float(lr) * np.sqrt(sd[str(n)].numel())
        assert abs(got_s[2] - row[2]) <= 2e-3 * row[2] + slack + 1e-6, f"post {n}: {got_s} vs {row}"
    tsd = teacher.state_dict()
    for n, row in zip(g["teacher_post_names"], g["teacher_post_stats"]):
        if str(n) in NOISE_DOMINATED:
            continue
        got_s = stat(tsd[str(n)])
        slack = 2.0 * float(lr) * (1 - float(mom)) * np.sqrt(tsd[str(n)].numel())
        assert abs(got_s[2] - row[2]) <= 1e-4 * row[2] + slack + 1e-6, f"ema {n}: {got_s} vs {row}"
    return worst


def check_small_steps(device, loss_tol=1e-3):
    """BASELINE config #1: CCD_pretrain_ViT_small hyper-parameters, B=8, two consecutive iterations vs the reference."""
    g = np.load(os.path.join(GOLD, "small_step.npz"))
    torch.manual_seed(0)
    np.random.seed(0)
    student, teacher = pretrain.build_networks(arch="vit_small", out_dim=65536, drop_path_rate=0.0,
                                               norm_last_layer=False, device=device)
    sd = student.state_dict()
    for n, row in zip(g["init_names"], g["init_stats"]):
        assert_init_stat(stat(sd[str(n)]), row, n)
    dino_loss = DINOLoss(65536, 2, 0.04, 0.04, 0, 40).to(device)
    opt = pretrain.make_optimizer(student, clip_grad=3.0)
    report = {}
    # The reference's trajectory after the first update depends on an amplified rounding residue (see NOISE_DOMINATED and
    # oracle.dino_head_forward(exact_zero_rows=...)): exp(log_softmax(0)) - softmax(0) = -2.3e-12 per logit of an exactly-uniform row,
    # a property of the platform's fp32 expf / logf that F.normalize's backward multiplies by 1 / eps = 1e12.  It is deterministic on
    # one platform - tests/golden/small_step_ref_noise.json (tools/gen_golden.py --only small_noise): the REAL reference's iteration-1
    # loss does not move by more than 2e-6 under 1 / 2 / 4 / 8 threads or permutations of the 65 536 output units - and it is gone
    # when the reference's loss evaluates its log-softmax in float64: iteration 1 then lands 9.3e-3 away, where the exact oracle and
    # the HIP path land.  From iteration 1 on the gates are therefore (a) the CPU oracle with that single residue removed, (b) the
    # real reference with float64 log-softmax, both at `loss_tol`, and (c) the recorded fp32 reference within the measured shift.
    import json
    with open(os.path.join(GOLD, "small_step_ref_noise.json")) as f:
        ref_noise = json.load(f)
    from oracle import ccd_oracle as O
    o_student, o_teacher = O.build_pair(O.Spec(norm_last_layer=False, **O.ARCH["vit_small"]), seed=0)
    o_center, o_opt = torch.zeros(1, 65536), O.AdamWState()
    for step in range(2):
        p = f"s{step}/"
        epoch, lr, wd, mom, clip, freeze, seed = g[p + "hyper"]
        images, masks, metrics = make_batch(8, seed=int(seed), device=device)
        captured = {}
        orig = student.forward

        def spy(*a, **k):
            out = orig(*a, **k)
            captured["out"] = out
            return out

        student.forward = spy
        loss = pretrain.training_iteration(student, teacher, dino_loss, opt, images, masks, metrics, int(epoch), lr, wd,
                                           mom, freeze_last_layer=int(freeze))
        student.forward = orig
        out = captured["out"]
        sel = out.raw("selection")
        np.testing.assert_array_equal(sel.idmap.cpu().numpy(), g[p + "zero_idmap"])          # bit-exact index map
        np.testing.assert_array_equal(out["index"].cpu().numpy(), g[p + "new_index"])
        losses = np.array([loss.item(), dino_loss.last_losses["mask_loss"].item(),
                           dino_loss.last_losses["Dino_loss"].item()])
        rec = O.train_iteration(o_student, o_teacher, o_center, o_opt, make_batch(8, seed=int(seed)), int(epoch), lr, wd,
                                mom, freeze_last_layer=int(freeze), exact_zero_rows=True)
        o_center = rec["center"]
        exact = np.array([rec["loss"], rec["mask_loss"], rec["dino_loss"]])
        report[f"step{step}"] = {"hip": losses.tolist(), "reference": g[p + "losses"].tolist(),
                                 "oracle_exact_zero_rows": exact.tolist()}
        np.testing.assert_allclose(losses, exact, atol=loss_tol, rtol=0, err_msg=f"losses vs exact oracle, step {step}")
        if step == 1:
            ref64 = np.array(ref_noise["s1_losses_with_float64_log_softmax"])
            report["step1"]["reference_with_float64_log_softmax"] = ref64.tolist()
            np.testing.assert_allclose(losses, ref64, atol=loss_tol, rtol=0, err_msg="losses vs the reference with float64 log-softmax, step 1")
        shift = float(np.abs(np.array(ref_noise["s1_shift_fp32_vs_float64_log_softmax"])).max())       # 9.3e-3, measured
        ref_tol = loss_tol if step == 0 else shift + loss_tol
        np.testing.assert_allclose(losses, g[p + "losses"], atol=ref_tol, rtol=0, err_msg=f"losses vs reference, step {step}")
        r, c = g[p + "rows"], g[p + "cols"]
        sl = out["instances_view"].detach().float()[torch.as_tensor(r)][:, torch.as_tensor(c)].cpu().numpy()
        assert np.abs(sl - g[p + "student_logits_sample"]).max() < 3e-2
        if step == 0:
            np.testing.assert_allclose(dino_loss.center[0, torch.as_tensor(c)].cpu().numpy(), g[p + "center_sample"],
                                       atol=2e-3)
        cdiff = float(np.abs(dino_loss.center.cpu().numpy() - o_center.numpy()).max())
        report[f"step{step}"]["center_max_abs_diff_vs_exact_oracle"] = cdiff
        assert cdiff < 3e-3, cdiff
        arena = student.arena
        for n, row in zip(g[p + "grad_names"], g[p + "grad_stats"]):
            name = str(n)
            got_l2 = arena.g(name).double().pow(2).sum().sqrt().item()
            # (a) every tensor against the CPU oracle run with exactly-zero rows carrying no gradient
            want_l2 = rec["grads_raw"][name].double().pow(2).sum().sqrt().item()
            if want_l2 > 1e-5:
                assert abs(got_l2 - want_l2) <= 8e-2 * want_l2, f"step {step} grad norm {name}: {got_l2} vs oracle {want_l2}"
            # (b) first iteration also against the recorded reference numbers (bar its three noise-amplified tensors)
            if step == 0 and name not in NOISE_DOMINATED and row[2] > 1e-5:
                assert abs(got_l2 - row[2]) <= 8e-2 * row[2], f"step 0 grad norm {name}: {got_l2} vs reference {row[2]}"
    return report


def check_small3_steps(device, loss_tol=1e-3):
    """Multi-iteration parity against the REAL reference (tests/golden/small3_step.npz): CCD_pretrain_ViT_small, B=8,
    head biases perturbed to non-zero values before the first step - so no pooled row enters F.normalize as an exact zero
    vector and none of the reference's gradients is rounding residue times 1/eps - and the last layer of the segmentation
    head fitted to the text masks (recorded in the fixture), so that the predicted-mask branch thresholds logits with real
    margins.  One iteration on the predicted-mask branch (epoch 30, dino_vision.py:64-70) followed by three consecutive
    iterations on the dataset-mask branch.  At EVERY iteration: distillation / mask / total loss within `loss_tol` (1e-3, the
    north star's tolerance), the character-mask index map and `new_index` BIT-EXACT, every gradient norm within 8 %, no
    tensor excluded.  On the predicted-mask branch the model's own bf16-path prediction must equal the reference's fp32
    prediction pixel for pixel (flips would only be tolerated where the reference's margin is inside the measured logit
    error - with this fixture there is no such pixel); the same iteration is also run with the reference's prediction
    injected, which isolates everything behind the threshold."""
    from ccd_amd import ops
    from ccd_amd.synthetic import make_text_like_batch
    g = np.load(os.path.join(GOLD, "small3_step.npz"))

    def build():
        torch.manual_seed(0)
        np.random.seed(0)
        student, teacher = pretrain.build_networks(arch="vit_small", out_dim=65536, drop_path_rate=0.0,
                                                   norm_last_layer=False, device=device)
        gen = torch.Generator().manual_seed(int(g["perturb"][0]))
        tsd = teacher.state_dict()
        with torch.no_grad():
            for k, v in student.state_dict().items():
                if k.startswith("head.") and k.endswith(".bias"):
                    v.add_((float(g["perturb"][1]) * torch.randn(v.shape, generator=gen)).to(v.device))
                    tsd[k].copy_(v)
        sd = student.state_dict()
        for n, row in zip(g["init_names"], g["init_stats"]):
            assert_init_stat(stat(sd[str(n)]), row, n)
        with torch.no_grad():
            sd["segmentation.cls.weight"].copy_(torch.from_numpy(g["cls_weight"]).to(device))
            sd["segmentation.cls.bias"].copy_(torch.from_numpy(g["cls_bias"]).to(device))
        if getattr(student, "arena", None) is not None:
            student.arena.refresh_mirrors()
        return student, teacher, DINOLoss(65536, 2, 0.04, 0.04, 0, 40).to(device), pretrain.make_optimizer(student, clip_grad=3.0)

    def iteration(nets, step, inject_reference_prediction=False):
        student, teacher, dino_loss, opt = nets
        p = f"s{step}/"
        epoch, lr, wd, mom, clip, freeze, seed = g[p + "hyper"]
        images, masks, metrics = (make_text_like_batch if epoch >= 30 else make_batch)(8, seed=int(seed), device=device)
        captured = {}
        orig = student.forward
        student.forward = lambda *a, **k: captured.setdefault("out", orig(*a, **k))
        real_seg_to_mask = ops.seg_to_mask
        if inject_reference_prediction:
            ref_pred = torch.from_numpy(g[p + "pred_mask"].astype(np.float32)).to(device)
            ops.seg_to_mask = lambda seg, B: ref_pred.clone()
        try:
            loss = pretrain.training_iteration(student, teacher, dino_loss, opt, images, masks, metrics, int(epoch), lr, wd,
                                               mom, freeze_last_layer=int(freeze))
        finally:
            student.forward = orig
            ops.seg_to_mask = real_seg_to_mask
        out = captured["out"]
        losses = np.array([loss.item(), dino_loss.last_losses["mask_loss"].item(), dino_loss.last_losses["Dino_loss"].item()])
        rep = {"epoch": int(epoch), "hip": losses.tolist(), "reference": g[p + "losses"].tolist(),
               "abs_diff": np.abs(losses - g[p + "losses"]).tolist()}
        idmap = out.raw("selection").idmap.cpu().numpy()
        if epoch >= 30 and not inject_reference_prediction:
            seg_ref = g[p + "seg_logits_view1"]
            margin = np.abs(seg_ref[:, 1] - seg_ref[:, 0])
            seg = out["mask"].detach().float()[:8].cpu().numpy()
            flips = (seg[:, 1] > seg[:, 0]).astype(np.uint8) != g[p + "pred_mask"]
            rep["pred_mask_flipped_pixels"] = int(flips.sum())
            rep["seg_logit_max_abs_err"] = float(np.abs(seg - seg_ref).max())
            rep["reference_margin_min"] = float(margin.min())
            print(f"small3 step {step} (epoch {int(epoch)}): {rep['pred_mask_flipped_pixels']} of {flips.size} predicted-mask pixels "
                  f"flipped, max logit error {rep['seg_logit_max_abs_err']:.4f}, smallest reference margin {margin.min():.4f}")
            assert not (flips & (margin > 2.0 * rep["seg_logit_max_abs_err"])).any(), "prediction differs beyond the logit error"
            assert rep["pred_mask_flipped_pixels"] == 0, "the fixture has margins: the bf16 path must reproduce the prediction"
        np.testing.assert_array_equal(idmap, g[p + "zero_idmap"])                              # bit-exact index map
        np.testing.assert_array_equal(out["index"].cpu().numpy(), g[p + "new_index"])
        np.testing.assert_allclose(losses, g[p + "losses"], atol=loss_tol, rtol=0, err_msg=f"losses vs reference, step {step}")
        r, c = g[p + "rows"], g[p + "cols"]
        sl = out["instances_view"].detach().float()[torch.as_tensor(r)][:, torch.as_tensor(c)].cpu().numpy()
        assert np.abs(sl - g[p + "student_logits_sample"]).max() < 4e-2
        arena = student.arena
        for n, row in zip(g[p + "grad_names"], g[p + "grad_stats"]):
            got_l2 = arena.g(str(n)).double().pow(2).sum().sqrt().item()
            if row[2] > 1e-5:
                assert abs(got_l2 - row[2]) <= 8e-2 * row[2], f"step {step} grad norm {n}: {got_l2} vs reference {row[2]}"
        return rep

    report = {}
    nets = build()
    for step in range(4):
        report[f"step{step}"] = iteration(nets, step)
    # the predicted-mask iteration once more on fresh networks with the REFERENCE's thresholded prediction handed to the branch:
    # connected components, warp, pooling, head, both losses and every gradient behind the threshold, at the same tolerances
    report["step0_reference_prediction_injected"] = iteration(build(), 0, inject_reference_prediction=True)
    return report


def check_fold_tap_matches_separate(device, E=384, batch=4, drop_path=0.3):
    """A tap's LayerNorm backward inside the qkv data-gradient product of the block above (engine.Fusion.fold_tap,
    ccd_gemm_nt_lnbwd_tap_g16) against the separate ccd_ln_bwd launch per tap: the same sums in another order - every gradient
    tensor agrees to the rounding of the bf16 stream, the norm_seg gradients (what the fold computes itself) tensor by tensor.

    The norm_seg gradients are small sums of the segmentation head's gradient d_tap, and d_tap itself differs from run to run by
    the order of atomic sums upstream: two runs of the SEPARATE path already differ by 0.5 - 1.5 % there.  So the fold's own
    contribution is checked on the d_tap it was handed, against the separate launch on the rows, statistics and gamma that the
    separate path hands ccd_ln_bwd in the other run: the engine's wiring of the fold and its sums, without the upstream noise."""
    from ccd_amd import engine, ops
    results = {}
    saved = engine.Fusion.fold_tap, ops.gemm_nt_lnbwd, ops.ln_bwd
    real_lnbwd, real_ln_bwd = ops.gemm_nt_lnbwd, ops.ln_bwd
    names = ["backbone.norm_seg.0.weight", "backbone.norm_seg.0.bias", "backbone.norm_seg.1.weight", "backbone.norm_seg.1.bias",
             "backbone.blocks.2.norm1.weight", "backbone.blocks.0.mlp.fc2.bias", "backbone.patch_embed.proj.weight"]
    tap_of = {}                     # data_ptr of a norm_seg.j weight gradient -> j (the current run's student)
    separate, folded = {}, {}       # j -> inputs of the separate launch (fold off) / what the fold was handed and added (fold on)

    def ln_bwd_traced(dy, x, mean, rstd, gamma, g, dgamma, dbeta, *args, **kw):
        j = tap_of.get(dgamma.data_ptr())
        if j is not None:
            separate[j] = (x.clone(), mean.clone(), rstd.clone(), gamma.clone())
        return real_ln_bwd(dy, x, mean, rstd, gamma, g, dgamma, dbeta, *args, **kw)

    def gemm_nt_lnbwd_traced(*args, tap=None, **kw):
        if tap is None:
            return real_lnbwd(*args, **kw)
        d_tap, tap_gamma, tap_dgamma, tap_dbeta = tap
        before = tap_dgamma.clone(), tap_dbeta.clone()
        out = real_lnbwd(*args, tap=tap, **kw)
        folded[tap_of[tap_dgamma.data_ptr()]] = (d_tap.clone(), tap_gamma.clone(), tap_dgamma - before[0], tap_dbeta - before[1])
        return out

    try:
        ops.gemm_nt_lnbwd, ops.ln_bwd = gemm_nt_lnbwd_traced, ln_bwd_traced
        for fold in (False, True):
            engine.Fusion.fold_tap = fold
            torch.manual_seed(5)
            np.random.seed(5)
            engine._DROPPATH_SEED.update(base=91, calls=0)
            student, teacher = pretrain.build_networks(
                arch=None, out_dim=512, drop_path_rate=drop_path, norm_last_layer=False, seg_channel=E,
                backbone_kwargs=dict(embed_dim=E, depth=4, num_heads=E // 64, out_indices=[1, 2, 4]),
                head_kwargs=dict(hidden_dim=256, bottleneck_dim=64), device=device)
            assert engine.Fusion.resolve_g16(E), "the fold rides on the bf16 gradient stream"
            tap_of.clear()
            tap_of.update({student.arena.g(f"backbone.norm_seg.{j}.weight").data_ptr(): j for j in range(3)})
            dino_loss = DINOLoss(512, 2, 0.04, 0.04, 0, 40).to(device)
            images, masks, metrics = make_batch(batch, seed=13, device=device)
            opt = pretrain.make_optimizer(student, clip_grad=3.0)
            loss = pretrain.training_iteration(student, teacher, dino_loss, opt, images, masks, metrics, 1, 2e-4, 0.05, 0.99)
            if device.type == "cuda":
                torch.cuda.synchronize()
            results[fold] = (loss.item(), student.arena.grad.clone(), {n: student.arena.g(n).clone() for n in names})
    finally:
        engine.Fusion.fold_tap, ops.gemm_nt_lnbwd, ops.ln_bwd = saved
        engine._DROPPATH_SEED.update(base=None, calls=0)
    (l0, g0, t0), (l1, g1, t1) = results[False], results[True]
    assert abs(l0 - l1) < 1e-5, (l0, l1)
    report = {"loss": [l0, l1], "rel_grad_all": ((g1 - g0).double().norm() / g0.double().norm()).item()}
    assert report["rel_grad_all"] < 1e-2, report
    # the taps behind blocks 1 and 2 fold into the products of blocks 2 and 3; the one behind the last block keeps its launch
    assert sorted(separate) == [0, 1, 2] and sorted(folded) == [0, 1], (sorted(separate), sorted(folded))

    def rel(a, b):
        return ((a - b).double().norm() / b.double().norm().clamp_min(1e-30)).item()

    for n in names:
        report["rel_" + n] = rel(t1[n], t0[n])
        if not n.startswith("backbone.norm_seg."):
            assert report["rel_" + n] < 1e-2, (n, report["rel_" + n])
    for j, (d_tap, tap_gamma, dgamma, dbeta) in folded.items():
        x, mean, rstd, gamma = separate[j]
        assert torch.equal(gamma, tap_gamma), j
        want_g, want_b = torch.zeros_like(dgamma), torch.zeros_like(dbeta)
        real_ln_bwd(d_tap, x, mean, rstd, gamma, torch.zeros_like(d_tap), want_g, want_b, accumulate=False)
        if device.type == "cuda":
            torch.cuda.synchronize()
        for what, got, want in (("weight", dgamma, want_g), ("bias", dbeta, want_b)):
            key = f"rel_same_input_backbone.norm_seg.{j}.{what}"
            report[key] = rel(got, want)
            assert report[key] < 1e-4, (key, report[key])     # measured 4e-7 (weight) and 8e-8 (bias)
    return report


def check_mlp_bwd_fused_matches_two_launches(device, E=384, batch=4, depth=4, drop_path=0.3):
    """The MLP branch's data-gradient chain in one launch (engine.Fusion.mlp_bwd: ccd_proj_mlp_fused_gact in the forward pass,
    ccd_mlp_bwd_fused in the backward pass) against the gelu'(u) product + LayerNorm-backward product it replaces: the same losses
    (the forward pass only stores one more tensor), every gradient tensor to the rounding of the bf16 operands."""
    from ccd_amd import engine, ops
    results = {}
    saved = engine.Fusion.mlp_bwd
    names = ["backbone.blocks.0.mlp.fc1.weight", "backbone.blocks.0.mlp.fc1.bias", "backbone.blocks.1.mlp.fc2.weight",
             "backbone.blocks.1.norm2.weight", "backbone.blocks.1.norm2.bias", "backbone.blocks.0.attn.proj.bias",
             "backbone.blocks.0.attn.qkv.weight", "backbone.patch_embed.proj.weight"]
    launched = []
    real = ops.mlp_bwd_fused
    try:
        ops.mlp_bwd_fused = lambda *a, **k: (launched.append(1), real(*a, **k))[1]
        for fused in (False, True):
            engine.Fusion.mlp_bwd = fused
            torch.manual_seed(5)
            np.random.seed(5)
            engine._DROPPATH_SEED.update(base=91, calls=0)
            student, teacher = pretrain.build_networks(
                arch=None, out_dim=512, drop_path_rate=drop_path, norm_last_layer=False, seg_channel=E,
                backbone_kwargs=dict(embed_dim=E, depth=depth, num_heads=E // 64, out_indices=[1, 2, depth]),
                head_kwargs=dict(hidden_dim=256, bottleneck_dim=64), device=device)
            assert engine.Fusion.resolve_mlp_bwd(E, 4 * E) == fused
            dino_loss = DINOLoss(512, 2, 0.04, 0.04, 0, 40).to(device)
            images, masks, metrics = make_batch(batch, seed=13, device=device)
            opt = pretrain.make_optimizer(student, clip_grad=3.0)
            n0 = len(launched)
            loss = pretrain.training_iteration(student, teacher, dino_loss, opt, images, masks, metrics, 1, 2e-4, 0.05, 0.99)
            if device.type == "cuda":
                torch.cuda.synchronize()
            assert len(launched) - n0 == (depth if fused else 0), "one ccd_mlp_bwd_fused launch per block"
            results[fused] = (loss.item(), student.arena.grad.clone(), {n: student.arena.g(n).clone() for n in names})
    finally:
        ops.mlp_bwd_fused = real
        engine.Fusion.mlp_bwd = saved
        engine._DROPPATH_SEED.update(base=None, calls=0)
    (l0, g0, t0), (l1, g1, t1) = results[False], results[True]
    assert abs(l0 - l1) < 1e-5, (l0, l1)
    report = {"loss": [l0, l1], "rel_grad_all": ((g1 - g0).double().norm() / g0.double().norm()).item()}
    assert report["rel_grad_all"] < 1e-2, report
    for n in names:
        rel = ((t1[n] - t0[n]).double().norm() / t0[n].double().norm().clamp_min(1e-30)).item()
        report["rel_" + n] = rel
        assert rel < 1e-2, (n, rel)
    return report


def check_g_bf16_matches_fp32(device, E=128, batch=2, drop_path=0.3):
    """The backward pass with its residual-gradient stream as a bf16 tensor (engine.Fusion.g_bf16, ccd_*_g16) against the fp32
    stream: the forward pass and the losses are the same computation, every gradient tensor agrees to bf16 rounding of ONE stream
    (relative L2 error of the whole gradient arena, and of the tensors at the far end of the stream - the patch embedding)."""
    from ccd_amd import engine
    results = {}
    saved = engine.Fusion.g_bf16
    try:
        for g16 in (False, True):
            engine.Fusion.g_bf16 = g16
            torch.manual_seed(3)
            np.random.seed(3)
            engine._DROPPATH_SEED.update(base=77, calls=0)
            student, teacher = pretrain.build_networks(
                arch=None, out_dim=512, drop_path_rate=drop_path, norm_last_layer=False, seg_channel=E,
                backbone_kwargs=dict(embed_dim=E, depth=3, num_heads=E // 64, out_indices=[1, 2, 3]),
                head_kwargs=dict(hidden_dim=256, bottleneck_dim=64), device=device)
            assert engine.Fusion.resolve_g16(E) == g16
            dino_loss = DINOLoss(512, 2, 0.04, 0.04, 0, 40).to(device)
            images, masks, metrics = make_batch(batch, seed=11, device=device)
            opt = pretrain.make_optimizer(student, clip_grad=3.0)
            loss = pretrain.training_iteration(student, teacher, dino_loss, opt, images, masks, metrics, 1, 2e-4, 0.05, 0.99)
            if device.type == "cuda":
                torch.cuda.synchronize()
            grads = {n: student.arena.g(n).clone() for n in ("backbone.patch_embed.proj.weight", "backbone.pos_embed",
                                                             "backbone.blocks.0.attn.qkv.weight", "backbone.blocks.2.mlp.fc1.weight")}
            results[g16] = (loss.item(), student.arena.grad.clone(), grads)
    finally:
        engine.Fusion.g_bf16 = saved
        engine._DROPPATH_SEED.update(base=None, calls=0)
    (l0, g0, t0), (l1, g1, t1) = results[False], results[True]
    assert abs(l0 - l1) < 1e-5, (l0, l1)          # (the same forward pass up to the order of its fp32 atomics)
    report = {"loss": [l0, l1], "rel_grad_all": ((g1 - g0).double().norm() / g0.double().norm()).item()}
    assert report["rel_grad_all"] < 1e-2, report
    for n in t0:
        rel = ((t1[n] - t0[n]).double().norm() / t0[n].double().norm().clamp_min(1e-30)).item()
        report["rel_" + n] = rel
        assert rel < 2e-2, (n, rel)
    return report


def check_no_grad_train_droppath(device, E=128, views=4):
    """A backbone in train() mode with drop_path > 0 run under no_grad (nothing saved, DropPath masks drawn): the one-launch
    block half cannot serve a dropped MLP branch without x_mid (CCD_EINVAL), so those blocks take the two-launch path - same
    tokens as with the fusion switched off, same DropPath seeds."""
    from ccd_amd import engine
    from ccd_amd.modules import vision_transformer as vits
    torch.manual_seed(5)
    net = vits.VisionTransformer(patch_size=4, embed_dim=E, depth=3, num_heads=E // 64, mlp_ratio=4, qkv_bias=True, drop_path_rate=0.5,
                                 norm_layer=lambda e: torch.nn.LayerNorm(e, eps=1e-6), out_indices=[1, 2, 3]).to(device).train()
    net.ensure_arena()
    img = torch.randn((views, 3, 32, 128), generator=torch.Generator().manual_seed(1)).to(device)
    outs = []
    saved = engine.Fusion.proj_mlp
    try:
        for fused in (True, False):
            engine.Fusion.proj_mlp = fused
            engine._DROPPATH_SEED.update(base=1234, calls=0)
            with torch.no_grad():
                tokens, *taps = net.tokens_and_taps(img)
            outs.append([tokens.float().cpu()] + [t.float().cpu() for t in taps])
    finally:
        engine.Fusion.proj_mlp = saved
        engine._DROPPATH_SEED.update(base=None, calls=0)
    assert engine.Fusion.resolve_proj(E), "the embedding width must be one the fused block half takes"
    for a, b in zip(*outs):
        assert torch.isfinite(a).all()
        assert float((a - b).abs().max()) < 0.06, float((a - b).abs().max())      # bf16 LayerNorm outputs of O(1) values


def check_head_loss_fusion_matches_unfused(device, batch=4, out_dim=512):
    """One training iteration with the head's last product left to the loss (engine.LazyLogits -> ccd_head_loss_fwd / _bwd, the
    default where bottleneck_dim == 256) against the same iteration with the logits materialised (CCD_FUSE_HEAD_LOSS=0's chain):
    same losses, same centre, same update; the lazy output still hands out `instances_view` on request."""
    from ccd_amd import engine
    results = {}
    saved = engine.Fusion.head_loss
    try:
        for fused in (True, False):
            engine.Fusion.head_loss = fused
            torch.manual_seed(3)
            np.random.seed(3)
            student, teacher = pretrain.build_networks(
                arch=None, out_dim=out_dim, drop_path_rate=0.0, norm_last_layer=False, seg_channel=192,
                backbone_kwargs=dict(embed_dim=192, depth=3, num_heads=3, out_indices=[1, 2, 3]),
                head_kwargs=dict(hidden_dim=256, bottleneck_dim=256), device=device)
            dino_loss = DINOLoss(out_dim, 2, 0.04, 0.04, 0, 40).to(device)
            images, masks, metrics = make_batch(batch, seed=11, device=device)
            if fused:       # the forward pass alone: the student's logits are lazy, and can still be looked at
                s_out = student(images, metrics.float(), masks, 1, clusters=None)
                assert isinstance(s_out.raw("logits_buf"), engine.LazyLogits)
                view = s_out["instances_view"]
                assert view.shape[1] == out_dim and view.shape[0] == 2 * s_out.raw("selection").M
                engine._LAZY_LOGITS.clear()
            opt = pretrain.make_optimizer(student, clip_grad=3.0)
            w_init = student.arena.flat.clone()
            loss = pretrain.training_iteration(student, teacher, dino_loss, opt, images, masks, metrics, 1, 2e-4, 0.05, 0.99)
            if device.type == "cuda":
                torch.cuda.synchronize()
            results[fused] = (loss.item(), dino_loss.last_losses["Dino_loss"].item(), student.arena.grad.clone(),
                              student.arena.flat.clone() - w_init, dino_loss.center.clone())
            assert not engine._LAZY_LOGITS and not engine._BF16_LOGIT_GRADS, "a parked handle / gradient was left behind"
    finally:
        engine.Fusion.head_loss = saved
    (l1, d1, g1, u1, c1), (l0, d0, g0, u0, c0) = results[True], results[False]
    assert abs(l1 - l0) < 2e-5 and abs(d1 - d0) < 2e-5, (l1, l0, d1, d0)
    assert float((c1 - c0).abs().max()) < 1e-6
    rel_g = ((g1 - g0).double().norm() / g0.double().norm()).item()
    assert rel_g < 2e-2, rel_g          # bf16 logit gradients, rounded once in either chain
    rel_u = ((u1 - u0).double().norm() / u0.double().norm()).item()
    assert rel_u < 0.1, rel_u           # (Adam's first step: +-lr where the gradient's sign is rounding noise)
    return {"loss": [l1, l0], "dino": [d1, d0], "rel_grad": rel_g, "rel_update": rel_u}


def check_dist_world1(device, port=29611):
    """The N > 1 path on the one GPU there is: a 1-rank `nccl` (= RCCL) group, SyncBatchNorm conversion, DataParallel with
    its bucketed asynchronous all-reduces on a dedicated process group and reserved compute units, the centre all-reduce -
    every collective really issued (identities on one rank).  One iteration must equal the non-distributed one (up to the
    fp32-atomic summation order both runs share)."""
    import torch.distributed as dist
    from ccd_amd import ops, seghead
    from ccd_amd.parallel import DataParallel
    results = {}
    for mode in ("plain", "dist"):
        student, teacher = tiny_networks(device)
        dino_loss = DINOLoss(512, 2, 0.04, 0.04, 0, 40).to(device)
        images, masks, metrics = make_batch(4, seed=11, device=device)
        model = student
        calls = []
        if mode == "dist":
            dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                                    device_id=device if device.type == "cuda" else None)
            student = torch.nn.SyncBatchNorm.convert_sync_batchnorm(student)
            seghead.FORCE_SYNC = True
            model = DataParallel(student, reduce_at_world1=True, bucket_elems=1 << 18)
            assert model.reducer is not None and ops.policy_get("cu_reserve") == 8
            real = dist.all_reduce
            dist.all_reduce = lambda *a, **k: (calls.append(int(a[0].numel())), real(*a, **k))[1]
        try:
            opt = pretrain.make_optimizer(student, clip_grad=3.0)
            loss = pretrain.training_iteration(model, teacher, dino_loss, opt, images, masks, metrics, 1, 2e-4, 0.05, 0.99)
            if device.type == "cuda":
                torch.cuda.synchronize()
            results[mode] = (loss.item(), student.arena.flat.clone(), dino_loss.center.clone())
        finally:
            if mode == "dist":
                dist.all_reduce = real
                seghead.FORCE_SYNC = False
                ops.policy_set("cu_reserve", 0)
                dist.destroy_process_group()
        if mode == "dist":
            # gradient buckets (several, the arena is cut at 2^18 elements), 4 + 4 SyncBatchNorm exchanges, the centre
            assert sum(1 for n in calls if n >= 1 << 17) >= 2 and len(calls) >= 2 + 8 + 1, calls
    (l0, w0, c0), (l1, w1, c1) = results["plain"], results["dist"]
    assert abs(l0 - l1) < 1e-5, (l0, l1)
    # Adam's first step moves every element by ~lr whatever the gradient's size: where the true gradient is zero (e.g. the
    # key bias of qkv) the SIGN is rounding noise of fp32 atomics, different from run to run.  Compare the update as a whole.
    update = w0 - tiny_networks(device)[0].arena.flat
    rel = ((w0 - w1).double().norm() / update.double().norm()).item()
    # (a flipped sign moves an element by 2 lr: rel = 0.1 <=> 0.25 % of the elements flipped; measured 0.03 - 0.06 between two
    # runs whose atomics sum in another order - the reserved CUs change every persistent grid; a wrong reduction gives >= 0.5)
    assert rel < 0.1, f"the distributed iteration updated the weights differently (relative difference {rel})"
    assert (c0 - c1).abs().max().item() < 1e-6
    return {"loss_plain": l0, "loss_dist": l1, "collectives": len(calls)}


def check_full_batch_equals_micro_batches(device, B=256, mb=8):
    """BASELINE config #2's size, checked by more than isfinite: with BatchNorm in eval mode every image is independent, so
    the B = 256 forward pass + losses (512-view backbone launches, the worst-case-row head launch driven by the device-side
    row count, d_rows tile enumeration at M ~ 3.3 k) must reproduce the row-weighted mean of the same images run as 32
    micro-batches of 8 through the B = 8 path that the reference fixtures pin; M is recomputed on the host."""
    from ccd_amd import ops
    torch.manual_seed(0)
    np.random.seed(0)
    student, teacher = pretrain.build_networks(arch="vit_small", out_dim=65536, drop_path_rate=0.0,
                                               norm_last_layer=False, device=device)
    student.eval()
    teacher.eval()
    images, masks, metrics = make_batch(B, seed=77, device=device)

    def run(sl):
        dino_loss = DINOLoss(65536, 2, 0.04, 0.04, 0, 40).to(device)          # fresh centre for every call
        with torch.no_grad():
            s_out = student(images[sl], metrics[sl].float(), masks[sl], 1, clusters=None)
            t_out = teacher(images[sl], metrics[sl].float(), None, None, clusters=s_out["zero"], index=None)
            s_out["gt"] = [masks[sl], ops.warp_idmap(ops.mask_to_idmap(masks[sl].contiguous().float()), metrics[sl].contiguous())]
            dino_loss(s_out, t_out, 1)
        m = int(s_out.raw("selection").total.item())
        return dino_loss.last_losses["mask_loss"].item(), dino_loss.last_losses["Dino_loss"].item(), m

    mask_full, dino_full, m_full = run(slice(0, B))
    # M on the host: rows per view = sum over images of min(#components of the mask, 26 planes, clamp 3) + 1
    from oracle import ccl_np
    ids = np.stack([ccl_np.label_idmap(m) for m in masks.cpu().numpy()])
    counts = [len(set(np.unique(i).tolist()) - {255}) for i in ids]
    m_host = sum(min(max(c, 3), 26) + 1 if c < 26 else 26 for c in counts)
    assert m_full == m_host, (m_full, m_host)
    acc_mask = acc_dino = 0.0
    m_sum = 0
    for lo in range(0, B, mb):
        ml, dl, m = run(slice(lo, lo + mb))
        acc_mask += ml * mb
        acc_dino += dl * m
        m_sum += m
    assert m_sum == m_full
    assert abs(mask_full - acc_mask / B) < 1e-3, (mask_full, acc_mask / B)
    assert abs(dino_full - acc_dino / m_sum) < 1e-3, (dino_full, acc_dino / m_sum)
    # and one real training iteration at this size: finite, and it moves the loss it optimises
    student.train()
    dino_loss = DINOLoss(65536, 2, 0.04, 0.04, 0, 40).to(device)
    opt = pretrain.make_optimizer(student, clip_grad=3.0)
    l0 = pretrain.training_iteration(student, teacher, dino_loss, opt, images, masks, metrics, 1, 5e-4, 0.04, 0.9995).item()
    l1 = pretrain.training_iteration(student, teacher, dino_loss, opt, images, masks, metrics, 1, 5e-4, 0.04, 0.9995).item()
    assert np.isfinite([l0, l1]).all() and l1 < l0, (l0, l1)
    return {"M": m_full, "mask_loss": [mask_full, acc_mask / B], "dino_loss": [dino_full, acc_dino / m_sum], "train": [l0, l1]}


def check_properties_full_size(device, B=256):
    """Size-independent properties at BASELINE's full batch (where the oracle is too slow to be the checker)."""
    from ccd_amd import engine, ops
    images, masks, metrics = make_batch(B, seed=5, device=device)
    ids = ops.ccl_label(masks)
    # round trip through the reference's dense representation
    assert torch.equal(ops.planes_to_idmap(ops.idmap_to_planes(ids)), ids)
    # identity warp is the identity map; labelling a relabelled map is idempotent
    eye = torch.eye(3, device=device).repeat(B, 1, 1)
    assert torch.equal(ops.warp_idmap(ids, eye), ids)
    relabel = ops.ccl_label((ids != 255).float())
    assert torch.equal(relabel, ids)
    # planes are ordered left to right: mean column of plane k is non-decreasing in k
    idn = ids.cpu().numpy()
    xs = np.arange(128)[None, None, :]
    for b in range(0, B, 37):
        means = [(xs * (idn[b:b + 1] == k)).sum() / max((idn[b] == k).sum(), 1) for k in range(26) if (idn[b] == k).any()]
        assert means == sorted(means)
    # attention with V == 1 returns 1 (softmax rows sum to one), any Q/K
    E, heads = 384, 6
    qkv = torch.randn(64, 256, 3 * E, device=device, dtype=torch.bfloat16)
    qkv[..., 2 * E:] = 1.0
    out, _ = ops.attention_fwd(qkv, heads, 0.125)
    assert (out.float() - 1.0).abs().max() < 1e-2
    # region pooling is linear in the features
    sel = engine.Selection(torch.cat([ids, ops.warp_idmap(ids, metrics)]), B)
    f1 = torch.randn(2 * B, 256, E, device=device, dtype=torch.bfloat16)
    f2 = torch.randn(2 * B, 256, E, device=device, dtype=torch.bfloat16)
    pool = lambda f: engine.RegionPoolFn.apply(f, sel).float()
    assert (pool(f1) + pool(f2) - pool((f1.float() + f2.float()).to(torch.bfloat16))).abs().max() < 8e-2
    # optimizer: zero learning rate leaves the weights untouched; EMA with momentum 1 leaves the teacher untouched
    return int(sel.M)


def check_checkpoint_resume(device, tmp_path):
    """Checkpoint in the reference's layout (train.py:190-200: DDP-prefixed student/teacher, AdamW state, DINOLoss
    centre), restored into freshly built networks with restart_from_checkpoint: the next iteration is identical."""
    from ccd_amd.modules import utils
    from ccd_amd.parallel import DataParallel

    def build():
        student, teacher = tiny_networks(device)
        s, t = DataParallel(student), DataParallel(teacher)
        t.module.backbone.load_state_dict(s.module.backbone.state_dict())
        t.module.head.load_state_dict(s.module.head.state_dict())
        t.module.ensure_arena()
        loss = DINOLoss(512, 2, 0.04, 0.04, 0, 40).to(device)
        return s, t, loss, pretrain.make_optimizer(s.module, clip_grad=3.0)

    def run(s, t, loss, opt, seed, epoch):
        images, masks, metrics = make_batch(1, seed=seed, device=device)
        return float(pretrain.training_iteration(s, t, loss, opt, images, masks, metrics, epoch, 2e-4, 0.05, 0.99).item())

    s, t, loss, opt = build()
    run(s, t, loss, opt, seed=21, epoch=1)
    path = os.path.join(str(tmp_path), "checkpoint.pth")
    torch.save({"student": s.state_dict(), "teacher": t.state_dict(), "optimizer": opt.state_dict(), "epoch": 1,
                "iteration": 1, "dino_loss": loss.state_dict()}, path)
    keys = list(torch.load(path, map_location="cpu", weights_only=False)["student"])
    assert all(k.startswith("module.") for k in keys) and "module.backbone.blocks.0.attn.qkv.weight" in keys
    snap = {"flat": s.module.arena.flat.clone(), "tflat": t.module.arena.flat.clone(), "m": opt.exp_avg.clone(),
            "v": opt.exp_avg_sq.clone(), "steps": dict(opt.steps), "center": loss.center.clone(),
            "buffers": {k: v.clone() for k, v in s.module.named_buffers()}}
    want = run(s, t, loss, opt, seed=22, epoch=1)

    torch.manual_seed(99)                                      # different initial weights: everything must come from the file
    s2, t2, loss2, opt2 = build()
    restored = {"epoch": 0, "iteration": 0}
    utils.restart_from_checkpoint(path, run_variables=restored, student=s2, teacher=t2, optimizer=opt2, dino_loss=loss2)
    assert restored == {"epoch": 1, "iteration": 1}
    s2.module.ensure_arena()
    t2.module.ensure_arena()
    # the restored state is bit-identical to the state that was saved ...
    assert torch.equal(s2.module.arena.flat, snap["flat"]) and torch.equal(t2.module.arena.flat, snap["tflat"])
    assert torch.equal(opt2.exp_avg, snap["m"]) and torch.equal(opt2.exp_avg_sq, snap["v"]) and dict(opt2.steps) == snap["steps"]
    assert torch.equal(loss2.center, snap["center"])
    for k, v in s2.module.named_buffers():
        assert torch.equal(v, snap["buffers"][k]), k
    # ... and the next iteration reproduces the original run's loss (parameters only up to the fp32-atomic summation
    # noise that two identical runs show as well - Adam turns sign flips of zero-gradient elements into +-lr moves)
    got = run(s2, t2, loss2, opt2, seed=22, epoch=1)
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (got, want)


# ------------------------------------------------------------------------------------------------ finetune path
FT_WORDS = ["hello", "Wor1d!", "MI355X", "a", "text-recognition", "CCD", "~{unknown}", "0123456789abcdefghijklmnopqrstuvwxyz"]


def _register_test_arch():
    """A 2-block E=192 backbone under the name 'vit_test2' (DINO_Finetune looks architectures up by name)."""
    from functools import partial
    import torch.nn as nn
    from ccd_amd.modules import vision_transformer as vits
    if "vit_test2" not in vits.__dict__:
        vits.vit_test2 = lambda patch_size=16, **kw: vits.VisionTransformer(
            patch_size=patch_size, embed_dim=192, depth=2, num_heads=3, mlp_ratio=4, qkv_bias=True,
            norm_layer=partial(nn.LayerNorm, eps=1e-6), **kw)
    if "vit_test128" not in vits.__dict__:      # E % 128 == 0: the MLP branch runs on the fused kernel (mlp_fused.h)
        vits.vit_test128 = lambda patch_size=16, **kw: vits.VisionTransformer(
            patch_size=patch_size, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True,
            norm_layer=partial(nn.LayerNorm, eps=1e-6), **kw)


def _cosine(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


def check_finetune_against_oracle(device, arch="vit_test2", vit_kw=None, n_layers=2, B=3, steps=2, loss_tol=2e-3,
                                  decode=True, max_seq_len=25):
    """Product (HIP kernels) vs the pinned CPU oracle on the same seed / inputs: initial weights bit-identical, loss,
    logits, attention map, every gradient, AdamW-updated weights, greedy decoding."""
    from ccd_amd import finetune as ft
    from oracle import ccd_oracle as O
    from oracle import finetune_oracle as FO
    _register_test_arch()
    vit_kw = vit_kw or dict(embed_dim=192, depth=2, heads=3)
    spec = FO.FtSpec(vit=O.Spec(**vit_kw), n_layers=n_layers, max_seq_len=max_seq_len)
    net = FO.init_finetune(spec, seed=5)
    torch.manual_seed(5)
    model = ft.build_model(ft.FinetuneConfig(arch=arch, drop_path_rate=0.0, decoder_n_layers=n_layers,
                                             decoder_max_seq_len=max_seq_len), device, dropout=0.0)
    sd = model.state_dict()
    assert set(sd) == set(net.P), set(sd) ^ set(net.P)
    for k, v in net.P.items():
        assert torch.equal(sd[k].detach().cpu().float(), v.detach()), f"init differs: {k}"
    opt = ft.make_optimizer(model)
    o_opt = O.AdamWState()
    targets = model.label_convertor.str2tensor(FT_WORDS[:B])
    assert torch.equal(targets, FO.str2tensor(FT_WORDS[:B], max_seq_len=max_seq_len))
    gen = torch.Generator().manual_seed(77)
    for step in range(steps):
        img = torch.randn(B, 3, 32, 128, generator=gen)
        lr = 3e-4
        rec = FO.train_iteration(net, o_opt, img, targets, lr)
        # forward pieces with gradients kept, then the optimizer step
        for g_ in opt.param_groups:
            g_["lr"] = lr
        loss, attn = model(img.to(device), targets.to(device), return_loss=True)
        opt.zero_grad()
        loss.backward()
        assert abs(loss.item() - rec["loss"]) < loss_tol, (step, loss.item(), rec["loss"])
        a_ref = rec["attn"]
        assert attn.shape == a_ref.shape
        assert (attn.float().cpu() - a_ref).abs().max() < 2e-2 * a_ref.max() + 1e-4
        worst = (1.0, "")
        for k, g_ref in rec["grads_raw"].items():
            got = model.arena.g(k).detach().cpu()
            nr = g_ref.norm().item()
            if nr < 1e-7:
                assert got.norm().item() < 1e-4, k
                continue
            c = _cosine(got, g_ref)
            worst = min(worst, (c, k))
            assert abs(got.norm().item() / nr - 1) < 8e-2, (step, k, got.norm().item(), nr)
        assert worst[0] > 0.97, worst
        for k in model.unused_parameter_names():
            assert float(model.arena.g(k).abs().max()) == 0.0 and k not in rec["grads_raw"], k
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        opt.step()
        after = model.state_dict()
        for k in rec["grads_raw"]:
            mine, ref = after[k].detach().cpu(), net.P[k].detach()
            # Adam's first steps move EVERY element by ~lr, also where only rounding noise decides the gradient's sign:
            # two implementations can be 2*lr apart per step there, and never more
            assert (mine - ref).abs().max() <= 2.2 * lr * (step + 1) + 1e-6, (k, (mine - ref).abs().max().item())
            moved = (ref - before[k].cpu()).abs() > 0.5 * lr
            if moved.any() and step == 0:
                agree = (torch.sign(mine - before[k].cpu()) == torch.sign(ref - before[k].cpu()))[moved].float().mean()
                assert agree > 0.9, (k, float(agree))
        assert all(torch.equal(before[k].cpu(), after[k].cpu()) for k in model.unused_parameter_names())
    if decode:
        img = torch.randn(B, 3, 32, 128, generator=gen)
        # decode with IDENTICAL weights: load the oracle's into the product
        model.load_state_dict({k: v.detach() for k, v in net.P.items()})
        model.eval()
        with torch.no_grad():
            probs = model(img.to(device), None, return_loss=False)
            ref = FO.forward_test(net.P, spec, img)
            _, logits_ref, _ = FO.forward_train(net.P, spec, img, targets)
            model.train()
            feat = model.extract_feat(img.to(device))
            logits, _ = model.decoder(feat, model.encoder(feat), {"padded_targets": targets.to(device)}, train_mode=True)
        assert probs.shape == ref.shape == (B, max_seq_len, 92)
        # the product decodes incrementally (one new position per step); the reference's full re-run is kept as a checker
        from ccd_amd import finetune_engine as fe
        model.eval()
        with torch.no_grad():
            full = fe.greedy_decode_full(model.decoder, model.encoder(model.extract_feat(img.to(device))))
        model.train()
        assert (full.cpu() - probs.cpu()).abs().max() < 5e-3, float((full.cpu() - probs.cpu()).abs().max())
        probs = probs.cpu()
        # greedy decoding feeds its own argmax back: compare a position only while the decoded prefixes agree
        same_prefix = torch.ones(B, dtype=torch.bool)
        compared = 0
        for t in range(max_seq_len):
            if same_prefix.any():
                d = (probs[same_prefix, t] - ref[same_prefix, t]).abs().max()
                assert d < 4e-2, (t, float(d))
                compared += int(same_prefix.sum())
            same_prefix &= probs[:, t].argmax(-1) == ref[:, t].argmax(-1)
        assert compared >= B * 4, compared
        assert (logits.float().cpu() - logits_ref).abs().max() < 6e-2 * max(1.0, logits_ref.abs().max().item())
        clear = ref.topk(2, -1).values
        clear = (clear[..., 0] - clear[..., 1]) > 0.1
        assert torch.equal(probs.cpu().argmax(-1)[clear], ref.argmax(-1)[clear])


def check_finetune_dropout(device, B=2, n_layers=1):
    """Training with the reference's dropout (p = 0.1): masks are a pure function of the seeds, so two runs with the same
    seeds are identical and the analytic gradient matches a central finite difference of the loss taken with the SAME
    seeds; eval mode switches dropout off."""
    from ccd_amd import finetune as ft
    _register_test_arch()
    torch.manual_seed(9)
    model = ft.build_model(ft.FinetuneConfig(arch="vit_test2", drop_path_rate=0.0, decoder_n_layers=n_layers,
                                             decoder_max_seq_len=12), device)
    targets = model.label_convertor.str2tensor(FT_WORDS[:B]).to(device)
    img = torch.randn(B, 3, 32, 128, generator=torch.Generator().manual_seed(3)).to(device)

    def reseed():
        for m in (model.encoder, model.decoder):
            m._base, m._calls = 12345, 0

    outs = []
    for rep in range(2):
        reseed()
        loss, _ = model(img, targets)
        model.arena.zero_grad()
        loss.backward()
        outs.append((loss.item(), model.arena.grad.clone()))
    assert abs(outs[0][0] - outs[1][0]) < 1e-5, (outs[0][0], outs[1][0])         # the loss sum uses fp32 atomics
    assert (outs[0][1] - outs[1][1]).abs().max() <= 1e-3 * outs[0][1].abs().max()      # fp32 atomics reorder sums
    model.eval()
    with torch.no_grad():
        l_eval, _ = model(img, targets)
    assert abs(l_eval.item() - outs[0][0]) > 1e-4                                      # dropout really was on
    model.train()
    name = "decoder.layer_stack.0.mlp.w_2.weight"
    g = model.arena.g(name).clone()
    w = model.arena.w(name)
    w0 = w.clone()
    direction = g / g.norm()
    eps = 2e-2
    vals = []
    for sgn in (+1, -1):
        w.copy_(w0 + sgn * eps * direction)
        model.arena.refresh_mirrors()
        reseed()
        with torch.no_grad():
            vals.append(model(img, targets)[0].item())
    w.copy_(w0)
    model.arena.refresh_mirrors()
    analytic = float((g * direction).sum())
    numeric = (vals[0] - vals[1]) / (2 * eps)
    assert abs(analytic - numeric) < 0.15 * abs(numeric) + 2e-3, (analytic, numeric)


def check_finetune_golden(device, tag="tiny", loss_tol=1e-3, report=None):
    """Product vs the REAL reference's recorded run (tests/golden/finetune_step.npz, tools/gen_golden.py): initial
    weights, two AdamW iterations (loss, attention map, every gradient norm), then greedy decoding.  -> report (losses of both
    sides, worst gradient-norm ratio per iteration) for profiles/."""
    report = {} if report is None else report      # (filled as it goes: the caller dumps it also when a gate below fails)
    report.update({"fixture": "finetune_step.npz/" + tag, "loss_tol": loss_tol, "steps": []})
    from ccd_amd import finetune as ft
    g = np.load(os.path.join(GOLD, "finetune_step.npz"))
    arch, n_layers, B = {"tiny": ("vit_tiny", 2, 4), "small": ("vit_small", 6, 8)}[tag]
    torch.manual_seed(0)
    model = ft.build_model(ft.FinetuneConfig(arch=arch, drop_path_rate=0.0, decoder_n_layers=n_layers), device, dropout=0.0)
    sd = model.state_dict()
    for n, row in zip(g[f"{tag}/init_names"], g[f"{tag}/init_stats"]):
        assert_init_stat(stat(sd[str(n)]), row, n)
    targets = model.label_convertor.str2tensor([str(w) for w in g["words"][:B]])
    np.testing.assert_array_equal(targets.numpy(), g[f"{tag}/targets"])
    targets = targets.to(device)
    opt = ft.make_optimizer(model)
    gen = torch.Generator().manual_seed(1234)
    for step in range(2):
        p = f"{tag}/s{step}/"
        img = torch.randn(B, 3, 32, 128, generator=gen)
        np.testing.assert_allclose(stat(img), g[p + "image_stat"], rtol=1e-12)
        loss_ref, lr = g[p + "loss"]
        for grp in opt.param_groups:
            grp["lr"] = float(lr)
        loss, attn = model(img.to(device), targets, return_loss=True)
        opt.zero_grad()
        loss.backward()
        report["steps"].append({"loss_hip": float(loss.item()), "loss_reference": float(loss_ref), "delta": float(loss.item() - loss_ref)})
        assert abs(loss.item() - loss_ref) < loss_tol, (step, loss.item(), loss_ref)
        am = attn.float().mean(1).cpu().numpy()
        assert np.abs(am - g[p + "attn_mean"]).max() < 2e-2 * g[p + "attn_mean"].max() + 1e-4
        names = [str(n) for n in g[p + "grad_names"]]
        for n, row in zip(names, g[p + "grad_stats"]):
            got = stat(model.arena.g(n))
            if row[2] < 1e-7:
                assert got[2] < 1e-4, n
            else:
                assert abs(got[2] / row[2] - 1) < 8e-2, (step, n, got[2], row[2])
                worst = report["steps"][-1].get("worst_grad_norm_ratio", 1.0)
                if abs(got[2] / row[2] - 1) > abs(worst - 1):
                    report["steps"][-1]["worst_grad_norm_ratio"] = float(got[2] / row[2])
                    report["steps"][-1]["worst_grad_tensor"] = n
        assert set(names) == {n for n, q in model.named_parameters()} - set(model.unused_parameter_names())
        opt.step()
        lr_sum = float(sum(g[f"{tag}/s{i}/loss"][1] for i in range(step + 1)))
        for n, row in zip(g[p + "post_names"], g[p + "post_stats"]):
            t_ = model.state_dict()[str(n)]
            got = stat(t_)
            # Adam moves every element by ~lr per step whatever the gradient's size: sign noise bounds the difference
            assert abs(got[2] - row[2]) <= 2e-3 * row[2] + 0.5 * lr_sum * t_.numel() ** 0.5 + 1e-6, (step, n, got[2], row[2])
    img = torch.randn(B, 3, 32, 128, generator=gen)
    np.testing.assert_allclose(stat(img), g[f"{tag}/eval_image_stat"], rtol=1e-12)
    model.eval()
    with torch.no_grad():
        probs = model(img.to(device), None, return_loss=False).cpu()
    ref = torch.from_numpy(g[f"{tag}/test_probs"])
    same_prefix = torch.ones(B, dtype=torch.bool)
    compared = 0
    for t in range(25):
        if same_prefix.any():
            assert (probs[same_prefix, t] - ref[same_prefix, t]).abs().max() < 5e-2, t
            compared += int(same_prefix.sum())
        same_prefix &= probs[:, t].argmax(-1) == ref[:, t].argmax(-1)
    assert compared >= 4 * B, compared
    report["decoded_positions_compared"] = compared
    return report


def check_pretrain_arch_vs_oracle(device, arch="vit_base", B=4, out_dim=4096, loss_tol=1e-3, dims=None):
    """One pretraining iteration of another shipped architecture (BASELINE config #4: vit_base = E 512 / 8 heads, which
    takes the non-fused residual / LayerNorm kernels; vit_base_768 = the 768 / 12 shape that config names) against the
    pinned CPU oracle: index maps bit-exact, losses, every gradient norm, centre.  `dims` = (embed_dim, depth, heads, taps):
    an explicit shallow model of the same width (the CPU executor's version of the wide architectures)."""
    from oracle import ccd_oracle as O
    torch.manual_seed(0)
    np.random.seed(0)
    if dims is None:
        student, teacher = pretrain.build_networks(arch=arch, out_dim=out_dim, drop_path_rate=0.0, norm_last_layer=False,
                                                   device=device)
        spec = O.Spec(norm_last_layer=False, out_dim=out_dim, seg_in=O.ARCH[arch]["embed_dim"], **O.ARCH[arch])
    else:
        E, depth, heads, taps = dims
        student, teacher = pretrain.build_networks(
            arch=None, out_dim=out_dim, drop_path_rate=0.0, norm_last_layer=False, seg_channel=E,
            backbone_kwargs=dict(embed_dim=E, depth=depth, num_heads=heads, out_indices=list(taps)), device=device)
        spec = O.Spec(embed_dim=E, depth=depth, heads=heads, taps=tuple(taps), out_dim=out_dim, norm_last_layer=False, seg_in=E)
    o_student, o_teacher = O.build_pair(spec, seed=0)
    sd = student.state_dict()
    for k in o_student.trainable:
        assert torch.equal(sd[k].detach().cpu(), o_student.P[k].detach()), f"init differs: {k}"
    dino_loss = DINOLoss(out_dim, 2, 0.04, 0.04, 0, 40).to(device)
    opt = pretrain.make_optimizer(student, clip_grad=3.0)
    images, masks, metrics = make_batch(B, seed=21, device=device)
    captured = {}
    orig = student.forward
    student.forward = lambda *a, **k: captured.setdefault("out", orig(*a, **k))
    loss = pretrain.training_iteration(student, teacher, dino_loss, opt, images, masks, metrics, 1, 1e-4, 0.04, 0.9995)
    student.forward = orig
    rec = O.train_iteration(o_student, o_teacher, torch.zeros(1, out_dim), O.AdamWState(), make_batch(B, seed=21), 1, 1e-4,
                            0.04, 0.9995, exact_zero_rows=True)
    out = captured["out"]
    np.testing.assert_array_equal(out.raw("selection").idmap.cpu().numpy(), rec["s_out"]["idmap"])
    np.testing.assert_array_equal(out["index"].cpu().numpy(), rec["s_out"]["index"].numpy())
    got = np.array([loss.item(), dino_loss.last_losses["mask_loss"].item(), dino_loss.last_losses["Dino_loss"].item()])
    want = np.array([rec["loss"], rec["mask_loss"], rec["dino_loss"]])
    np.testing.assert_allclose(got, want, atol=loss_tol, rtol=0)
    assert float((dino_loss.center.cpu() - rec["center"]).abs().max()) < 3e-3
    for name, g_ref in rec["grads_raw"].items():
        want_l2 = g_ref.double().pow(2).sum().sqrt().item()
        got_l2 = student.arena.g(name).double().pow(2).sum().sqrt().item()
        if want_l2 > 1e-5 and name not in NOISE_DOMINATED:
            assert abs(got_l2 - want_l2) <= 8e-2 * want_l2, f"grad norm {name}: {got_l2} vs oracle {want_l2}"
    report = {"arch": arch, "B": B, "out_dim": out_dim, "hip": got.tolist(), "oracle": want.tolist(),
              "delta_vs_oracle": (got - want).tolist()}
    # ... and against ONE ITERATION OF THE REAL REFERENCE (tests/golden/arch_step.npz, tools/gen_golden.py::gen_arch: the same seed,
    # batch and hyper-parameters) where the fixture holds this configuration
    fx = os.path.join(GOLD, "arch_step.npz")
    if dims is None and os.path.isfile(fx):
        g = np.load(fx)
        p = arch + "/"
        if p + "hyper" in g.files and int(g[p + "hyper"][7]) == B and int(g[p + "hyper"][8]) == out_dim:
            np.testing.assert_array_equal(out.raw("selection").idmap.cpu().numpy(), g[p + "zero_idmap"])
            np.testing.assert_array_equal(out["index"].cpu().numpy(), g[p + "new_index"])
            np.testing.assert_allclose(got, g[p + "losses"], atol=loss_tol, rtol=0, err_msg=f"{arch}: losses vs the reference")
            assert float(np.abs(dino_loss.center.cpu().numpy() - g[p + "center_after"]).max()) < 3e-3
            worst = 0.0
            for n, row in zip(g[p + "grad_names"], g[p + "grad_stats"]):
                if str(n) in NOISE_DOMINATED or row[2] <= 1e-5:
                    continue
                got_l2 = student.arena.g(str(n)).double().pow(2).sum().sqrt().item()
                worst = max(worst, abs(got_l2 - row[2]) / row[2])
                assert abs(got_l2 - row[2]) <= 8e-2 * row[2], f"grad norm {n}: {got_l2} vs reference {row[2]}"
            report.update({"reference": g[p + "losses"].tolist(), "delta_vs_reference": (got - g[p + "losses"]).tolist(),
                           "worst_grad_norm_rel_err_vs_reference": worst, "index_maps": "bit-exact"})
    return report


def check_finetune_properties_full_size(device, B=512):
    """BASELINE config #5 at its full batch (vit_small, 6 layers, B = 512): size-independent properties.
    (a) the returned loss equals torch's TFLoss on the returned logits; (b) eval-mode attention rows sum to 1 and the
    counter-based dropout keeps ~90 %; (c) same seeds -> same loss, finite gradients everywhere they should be;
    (d) decoded probabilities sum to 1, the incremental decoder equals the reference schedule, forward_test_speed stops
    at sample 0's <EOS>."""
    import torch.nn.functional as F
    from ccd_amd import finetune as ft, finetune_engine as fe
    torch.manual_seed(0)
    model = ft.build_model(ft.FinetuneConfig(arch="vit_small", drop_path_rate=0.1), device)
    g = torch.Generator().manual_seed(8)
    img = torch.randn(B, 3, 32, 128, generator=g).to(device)
    words = ["".join(model.label_convertor.idx2char[int(c)] for c in torch.randint(0, 90, (int(n),), generator=g))
             for n in torch.randint(1, 30, (B,), generator=g)]                       # some longer than max_seq_len
    targets = model.label_convertor.str2tensor(words).to(device)
    pad = model.label_convertor.padding_idx
    # (a) + (b, eval)
    model.eval()
    feat = model.extract_feat(img)
    logits, attn = model.decoder(feat, model.encoder(feat), {"padded_targets": targets}, train_mode=True)
    loss = model.loss(logits, {"padded_targets": targets})
    ref = F.cross_entropy(logits.float()[:, :-1].reshape(-1, 92), targets[:, 1:].reshape(-1), ignore_index=pad)
    assert abs(loss.item() - ref.item()) < 1e-4, (loss.item(), ref.item())
    assert attn.shape == (B, 8, 25, 256) and (attn.sum(-1) - 1).abs().max() < 2e-3
    # (b, train) + (c)
    model.train()
    outs = []
    for rep in range(2):
        for m in (model.encoder, model.decoder):
            m._base, m._calls = 4242, 0
        from ccd_amd import engine
        engine._DROPPATH_SEED.update(base=77, calls=0)
        l, a = model(img, targets)
        model.arena.zero_grad()
        l.backward()
        outs.append(l.item())
    assert abs(outs[0] - outs[1]) < 1e-5, outs
    kept = (a != 0).float().mean().item()
    assert 0.89 < kept < 0.91, kept
    assert (a.sum(-1) - 1).abs().mean() < 0.05                                     # E[dropout(p)/0.9] = p
    grad = model.arena.grad
    assert torch.isfinite(grad).all()
    for n in ("backbone.patch_embed.proj.weight", "encoder.fc1.weight", "decoder.trg_word_emb.weight",
              "decoder.layer_stack.0.self_attn.linear_k.weight", "decoder.layer_stack.5.enc_attn.linear_v.weight",
              "decoder.classifier.bias"):
        assert float(model.arena.g(n).abs().max()) > 0, n
    assert float(model.arena.g("decoder.trg_word_emb.weight")[pad].abs().max()) == 0.0      # padding_idx row frozen
    for n in model.unused_parameter_names():
        assert float(model.arena.g(n).abs().max()) == 0.0, n
    # (d)
    model.eval()
    with torch.no_grad():
        probs = model(img, None, return_loss=False)
        enc = model.encoder(model.extract_feat(img))
        full = fe.greedy_decode_full(model.decoder, enc[:64])
        speed = model(img, None, return_loss=False, test_speed=True)
    assert probs.shape == (B, 25, 92) and (probs.sum(-1) - 1).abs().max() < 1e-4
    assert (full - probs[:64]).abs().max() < 5e-3
    n = speed.shape[1]
    assert torch.equal(speed, probs[:, :n])
    first = probs[0].argmax(-1).tolist()
    flat_hit = [int(probs[:, t].reshape(-1).argmax()) == 91 for t in range(25)]
    assert n == (flat_hit.index(True) + 1 if True in flat_hit else 25), (n, first)
