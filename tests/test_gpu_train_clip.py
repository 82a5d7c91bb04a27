"""`ClipTrainer`: train steps on patches of a streamed clip, and the command line's `--input ... --train-steps` on top of it.  An 8-frame
144 x 176 yuv420p clip in a Y4M file, a x2 model built as `driver.run_c1` builds its own (fp32), LR patches of 64 x 64 (the smallest
FlowNet2 takes), groups of 4 frames, one sample of 3 frames per group: two steps."""
import copy
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from video_super_resolution_amd import VSR, driver, optim, y4m  # noqa: E402
from video_super_resolution_amd.weights import fill_module_  # noqa: E402

H, W, T, S, FMT = 144, 176, 8, 2, "yuv420p"
KW = dict(patch=64, group=4, frames_per_sample=3, samples_per_group=1, seed=3)


@pytest.fixture(scope="module")
def clip_bytes():
    video = torch.from_numpy(driver.synthetic_video(T, H, W)).cuda().float()
    return driver.frames_to_pix(video, FMT).cpu().numpy()


@pytest.fixture(scope="module")
def clip(clip_bytes, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("train_clip") / "in.y4m")
    with y4m.Y4MWriter(path, (H, W), FMT, (25, 1), "left", False) as w:
        for fr in clip_bytes:
            w.write(fr)
    return path


@pytest.fixture(scope="module")
def base_model():
    m = fill_module_(VSR(upscale_factor=S).eval(), seed=0).cuda()
    m.precision = m.model.precision = "fp32"
    return m


def _trainer(base_model, **kw):
    m = copy.deepcopy(base_model)
    opt = optim.Adam(m.parameters(), lr=1e-3)
    return m, opt, driver.ClipTrainer(m, opt, (H, W), FMT, **{**KW, **kw})


@pytest.fixture(scope="module")
def trained(base_model, clip):
    """One run of the trainer over the file: (model before, model after, optimizer, trainer)."""
    m, opt, tr = _trainer(base_model)
    with y4m.Y4MReader(clip) as src:
        steps = tr.run_stream(src)
    return base_model, m, opt, tr, steps


def test_two_groups_give_two_steps_with_finite_losses(trained, clip_bytes):
    _, _, _, tr, steps = trained
    assert steps == 2 and tr.steps == 2
    assert tr.losses.shape == (2,) and np.isfinite(tr.losses).all() and (tr.losses > 0).all()
    assert tr.grad_norms is None                                   # the optimizer does not clip
    assert (tr.frames_in, tr.frames_skipped, tr.h2d_bytes) == (T, 0, T * clip_bytes.shape[1])
    # the tables are the draws of the seed, in order
    rng = np.random.RandomState(3)
    want = [driver.patch_table(rng, 1, 4, 3, (H, W), 128, S) for _ in range(2)]
    assert len(tr.tables) == 2 and all(np.array_equal(a, b) for a, b in zip(tr.tables, want))


def test_the_sr_net_moved_and_nothing_else_did(trained):
    before, after, _, _, _ = trained
    old = dict(before.named_parameters())
    moved = frozen = 0
    for name, p in after.named_parameters():
        same = torch.equal(p.detach().view(torch.int32), old[name].detach().view(torch.int32))
        if name.startswith("model."):
            if p.grad is not None and p.grad.any():   # (a block whose output has no consumer gets zeros: tests/test_gpu_train_step.py)
                assert not same, f"{name} received a gradient and did not change"
                moved += 1
        else:
            assert same, f"{name} lies outside the SR net and changed"
            frozen += 1
    assert moved >= 60 and frozen > 0   # (every conv / PReLU of the SR net with a live gradient)
    for (name, b), (_, a) in zip(before.named_buffers(), after.named_buffers()):
        assert torch.equal(a, b), name


def _hand_made_step(base_model, clip_bytes, table):
    """The trainer's first step by hand on a fresh copy: the first group's frames converted, the table's sample cut, one `train_item`."""
    m = copy.deepcopy(base_model)
    opt = optim.Adam(m.parameters(), lr=1e-3)
    m.train()
    coef = driver.pix_coefficients(FMT, "bt709", False, inverse=True)
    src = torch.empty((4, H, W, 3), dtype=torch.float32, device="cuda")
    for g in range(4):
        driver.pix_ingest(torch.from_numpy(clip_bytes[g]).cuda(), (H, W), FMT, coef, "left", lr_out=src[g])
    hr, lr = driver.patch_gather(src, table, 3, 128, S)
    data, target, high_frames = driver.patch_item(hr, lr, 0)
    return float(driver.train_item(m, opt, data, target, high_frames))


def test_a_hand_made_pass_reproduces_the_first_loss(trained, clip_bytes):
    """The hand-made pass twice measures its own run-to-run difference; the trainer agrees with it within that same difference (observed on
    an MI355X: LAB_NOTES.md, "Training on a real clip")."""
    base, _, _, tr, _ = trained
    a = _hand_made_step(base, clip_bytes, tr.tables[0])
    b = _hand_made_step(base, clip_bytes, tr.tables[0])
    got = float(np.float32(tr.losses[0]))
    print(f"first loss: hand-made {a!r} and {b!r} (difference {abs(a - b)!r}), trainer {got!r} (difference {abs(got - a)!r})")
    assert math.isfinite(a) and abs(got - a) <= abs(a - b)


def test_bicubic_decimation_runs_and_sees_other_lr_frames(trained, base_model, clip):
    _, _, _, tr, _ = trained
    _, _, bic = _trainer(base_model, decimate="bicubic")
    with y4m.Y4MReader(clip) as src:
        assert bic.run_stream(src, max_steps=1) == 1
    assert bic.frames_in == 4 and np.array_equal(bic.tables[0], tr.tables[0])
    assert np.isfinite(bic.losses).all() and bic.losses[0] != tr.losses[0]


def test_the_trainer_refuses_what_it_cannot_train_on(base_model):
    m = copy.deepcopy(base_model)
    opt = optim.Adam(m.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="smaller than the HR patch"):
        driver.ClipTrainer(m, opt, (120, W), FMT, patch=64)
    with pytest.raises(ValueError, match="frames_per_sample must be at least 3"):
        driver.ClipTrainer(m, opt, (H, W), FMT, patch=64, frames_per_sample=2)
    with pytest.raises(ValueError, match="cannot hold a sample"):
        driver.ClipTrainer(m, opt, (H, W), FMT, patch=64, frames_per_sample=5, group=4)
    with pytest.raises(ValueError, match="decimate must be"):
        driver.ClipTrainer(m, opt, (H, W), FMT, patch=64, decimate="area")


def test_command_line_trains_saves_and_takes_the_file_back(clip, tmp_path, capsys):
    save = str(tmp_path / "ckpt")
    driver.main(["--input", clip, "--train-steps", "2", "--patch", "64", "--scale", "2", "--group", "4", "--save", save])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["train_steps"] == 2 and len(line["loss"]) == 2 and all(math.isfinite(v) and v > 0 for v in line["loss"])
    assert line["input"] == clip and line["pix_fmt_in"] == FMT and line["frames"] == 4 and line["grad_norm"] is None
    assert (line["patch"], line["frames_per_sample"], line["group"], line["seed"], line["decimate"], line["loss_path"]) == \
        (64, 3, 4, 0, "nearest", "reference")
    path = line["checkpoint"]
    assert path == save + "/VSR_train-checkpoint.pth.tar"
    # tensors and plain containers only: the weights-only reader takes the file, and the model takes the weights
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(ckpt) == ["arch", "epoch", "optimizer", "optimizer_state", "state_dict"]
    assert ckpt["arch"] == "VSR" and ckpt["epoch"] == 1 and ckpt["optimizer"] is None and ckpt["optimizer_state"]["state"]
    m = fill_module_(VSR(upscale_factor=S).eval(), seed=0)
    seeded = {k: v.clone() for k, v in m.model.state_dict().items()}
    got = driver.load_checkpoint(m, path)   # untrusted
    assert sorted(got) == sorted(ckpt) and any(not torch.equal(v, seeded[k]) for k, v in m.model.state_dict().items())
    out = str(tmp_path / "out.y4m")
    driver.main(["--input", clip, "--scale", "2", "--checkpoint", path, "--output", out])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["weights"] == path and line["windows"] == T - 2
    with y4m.Y4MReader(out) as r:
        assert len(r) == T - 2 and r.shape == (S * H, S * W)
