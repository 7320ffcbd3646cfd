"""`optimizer: sgd` / `optimizer: lars` without a GPU and without kernels: the fp64 restatement of the two rules (tests/optim_checks.py)
against the reference's recorded iterations (tests/golden/optim_cases.npz), the checkpoint layouts, and the selection by name."""
import pytest
import torch

import optim_checks as oc


def test_restatement_matches_reference_fixture(golden_dir):
    oc.check_restatement_matches_fixture(golden_dir)


def test_fixture_covers_the_issue_cases(golden_dir):
    c = oc.load_cases(golden_dir)
    shapes = {n: c[f"p0/{i}"].shape for i, n in enumerate(c["names"])}
    assert len(shapes) >= 5 and c["iters"] >= 4
    assert any(len(s) == 2 for s in shapes.values()) and any(len(s) == 3 and s[0] == 1 for s in shapes.values())
    assert any(n.endswith(".bias") and len(s) == 1 for n, s in shapes.items())
    assert any("last_layer" in n for n in shapes) and c["never_used"] and set(c["never_used"]) <= set(shapes)
    assert len(set(c["lr"].tolist())) == c["iters"] and len(set(c["wd"].tolist())) == c["iters"]
    assert list(c["epoch"][:2] < c["freeze_last_layer"]) == [True, True] and bool((c["epoch"][2:] >= c["freeze_last_layer"]).all())
    assert any(not c[f"p0/{i}"].any() and i not in [c["names"].index(n) for n in c["never_used"]] for i in range(len(shapes)))
    for kind in oc.KINDS:
        norms = c[f"{kind}/gnorm/0"]
        assert (norms < float(c["clip"])).any() and (norms > float(c["clip"])).any()      # one tensor stays under the clip
        last = c["names"].index(next(n for n in shapes if "last_layer" in n))
        assert not bool(c[f"{kind}/has_state/1/{last}"]) and bool(c[f"{kind}/has_state/2/{last}"])
        unused = c["names"].index(c["never_used"][0])
        assert not bool(c[f"{kind}/has_state/{c['iters'] - 1}/{unused}"])
    assert c["layouts"]["lars"]["group_keys"][0] == sorted(["lr", "weight_decay", "momentum", "eta", "weight_decay_filter",
                                                            "lars_adaptation_filter", "params"])
    assert c["layouts"]["sgd"]["state_keys"] == ["momentum_buffer"] and c["layouts"]["lars"]["state_keys"] == ["mu"]


def test_restatement_tells_the_rules_apart(golden_dir):
    """The gate is tight enough to see a wrong rule: SGD's update is not LARS's, and dropping the clip or the adaptation shows."""
    c = oc.load_cases(golden_dir)
    i = 0                                                     # the clipped 2-D weight
    p, g = torch.from_numpy(c["p0/0"]), torch.from_numpy(c["g/0/0"])
    args = (p, torch.zeros(p.shape), g, float(c["lr"][0]), float(c["wd"][0]), p.dim())
    want = torch.from_numpy(c[f"lars/p/0/{i}"])
    oc.close64(want, oc.step64("lars", *args)[0], 1e-6, 1e-7, "lars")
    for wrong in (oc.step64("sgd", *args)[0], oc.step64("lars", *args, clip=0.0)[0], oc.step64("lars", *args[:-1], 1)[0]):
        with pytest.raises(AssertionError):
            oc.close64(want, wrong, 1e-6, 1e-7, "wrong rule")


def test_checkpoint_layouts_and_cross_kind_loads(golden_dir):
    oc.check_checkpoint_layouts(golden_dir)


def test_make_optimizer_selects_by_name():
    from ccd_amd import optim, pretrain
    assert pretrain.OPTIMIZERS == {"adamw": optim.FusedClipAdamW, "sgd": optim.FusedClipSGD, "lars": optim.FusedClipLARS}

    class NoArena:
        def ensure_arena(self):
            raise AssertionError("an unknown optimizer name must be refused before anything is built")

    with pytest.raises(NotImplementedError, match="nope"):
        pretrain.make_optimizer(NoArena(), name="nope")
    src = open(pretrain.__file__.replace("ccd_amd/pretrain.py", "train.py")).read()
    assert "name=config.optimizer" in src and "only the fused AdamW is implemented" not in src


def test_c_abi_declares_the_new_entry_points():
    from ccd_amd import _lib
    for name in ("ccd_seg_moments", "ccd_sgd_momentum", "ccd_lars"):
        assert name in _lib.SIGNATURES
