"""The Sinkhorn-Knopp fixtures (tests/golden/sinkhorn_cases.npz, written by tools/gen_sinkhorn_golden.py from the reference's own
DINOLoss.sinkhorn_knopp_teacher) against the two numpy restatements of tests/sinkhorn_np.py, and the host-side pieces of the
feature: the constructor's arguments and the YAML keys.  No kernel runs here."""
import numpy as np
import pytest

import sinkhorn_np as R


def test_fixture_file(golden_dir):
    import os
    cases = R.load_cases(golden_dir)
    assert os.path.getsize(os.path.join(golden_dir, R.FIXTURE)) < (1 << 20)
    assert len(cases) >= 6 and {c["temp"] for _, c in cases} == {0.04, 0.07} and {c["n"] for _, c in cases} == {1, 3}
    for name, c in cases:
        assert c["t"].dtype == np.float32 and c["ref"].dtype == np.float32 and c["f64"].dtype == np.float64, name
        assert c["t"].shape == c["ref"].shape == c["f64"].shape and np.abs(c["t"]).max() <= 1.0, name
        assert 1e-7 < c["noise"] < 1e-5, (name, c["noise"])        # a few fp32 roundings of an exponent of size 25
    assert any(c["t"].shape[1] % 4 for _, c in cases) and any(c["t"].shape[0] > 128 for _, c in cases)


def test_linear_restatement_equals_log_domain(golden_dir):
    """The reference's loop, restated in float64, against the potentials' softmax: the identity the kernels rest on."""
    for name, c in R.load_cases(golden_dir):
        lin = R.linear(c["t"], c["temp"], c["n"])
        log = R.restatement(c["t"], c["temp"], c["n"])
        assert np.abs(lin - log).max() <= 1e-13, (name, np.abs(lin - log).max())
        assert np.abs(log - c["f64"]).max() <= 1e-13, name              # what the fixture recorded
        np.testing.assert_allclose(log.sum(axis=1), 1.0, rtol=0, atol=1e-12)
        assert abs(R.potentials(c["t"], c["temp"], c["n"]).mean()) < 1e-12


def test_restatement_against_recorded_reference(golden_dir):
    for name, c in R.load_cases(golden_dir):
        want = R.restatement(c["t"], c["temp"], c["n"])
        assert R.deviation(c["ref"], want) <= 2.0 * c["noise"], (name, R.deviation(c["ref"], want), c["noise"])
        np.testing.assert_allclose(c["ref"], want, rtol=2.0 * c["noise"], atol=R.FLOOR, err_msg=name)


def test_restatement_is_finite_where_fp32_exp_overflows():
    g = np.random.default_rng(5)
    t = g.uniform(-5.0, 5.0, (24, 1000)).astype(np.float32)
    with np.errstate(all="ignore"):
        assert not np.isfinite(R.linear(t, 0.04, 3, dtype=np.float32)).all()
    q = R.restatement(t, 0.04, 3)
    assert np.isfinite(q).all() and np.abs(q.sum(axis=1) - 1.0).max() < 1e-12


def test_constructor_arguments_and_yaml_keys(tmp_path):
    from ccd_amd import pretrain
    from ccd_amd.loss.Dino_loss import DINOLoss, TEACHER_CENTERINGS
    from ccd_amd.utils.utils import Config
    assert TEACHER_CENTERINGS == ("center", "sinkhorn_knopp")
    plain = DINOLoss(16, 2, 0.04, 0.07, 3, 10)
    assert (plain.teacher_centering, plain.sinkhorn_iterations) == ("center", 3)
    assert sorted(plain.state_dict()) == ["center"] == sorted(DINOLoss(16, 2, 0.04, 0.07, 3, 10, 0.1, 0.9, "sinkhorn_knopp", 2).state_dict())
    for bad in ("sinkhorn", "softmax", "", None):
        with pytest.raises(ValueError):
            DINOLoss(16, 2, 0.04, 0.07, 3, 10, teacher_centering=bad)
    with pytest.raises(ValueError):
        DINOLoss(16, 2, 0.04, 0.07, 3, 10, teacher_centering="sinkhorn_knopp", sinkhorn_iterations=0)
    assert callable(DINOLoss.sinkhorn_knopp_teacher)
    base = ("global:\n  name: t\n  phase: train\n  stage: pretrain-vision\n  workdir: w\n  seed: 1\n"
            "out_dim: 64\ncrops_number: 2\nwarmup_teacher_temp: 0.04\nteacher_temp: 0.07\nwarmup_teacher_temp_epochs: 3\n")
    (tmp_path / "a.yaml").write_text(base)
    (tmp_path / "b.yaml").write_text(base + "teacher_centering: sinkhorn_knopp\nsinkhorn_iterations: 2\n")
    a, b = Config(str(tmp_path / "a.yaml")), Config(str(tmp_path / "b.yaml"))
    assert a.teacher_centering is None and a.sinkhorn_iterations is None              # the shipped template has no such key
    la, lb = pretrain.make_dino_loss(a, 10), pretrain.make_dino_loss(b, 10)
    assert (la.teacher_centering, la.sinkhorn_iterations) == ("center", 3)
    assert (lb.teacher_centering, lb.sinkhorn_iterations) == ("sinkhorn_knopp", 2)
    np.testing.assert_array_equal(la.teacher_temp_schedule, plain.teacher_temp_schedule)
    (tmp_path / "c.yaml").write_text(base + "teacher_centering: sinkhorn\n")
    with pytest.raises(ValueError):
        pretrain.make_dino_loss(Config(str(tmp_path / "c.yaml")), 10)
