"""GPU pre-processing kernel (vt_preprocess) against the oracle's restatement of the torchvision / pytorchvideo
transforms the reference composes. Real COCO-like content is not needed: smooth + noisy synthetic uint8 frames."""
import numpy as np
import pytest
import torch

from oracle import vitron_oracle as O


def _frames(shape, seed):
    g = torch.Generator().manual_seed(seed)
    F_, H, W = shape
    yy, xx = torch.meshgrid(torch.linspace(0, 3.0, H), torch.linspace(0, 5.0, W), indexing="ij")
    base = 127 + 90 * torch.sin(yy[None] * 2.1 + torch.arange(F_)[:, None, None]) * torch.cos(xx[None] * 1.3)
    img = base[..., None] + torch.randn((F_, H, W, 3), generator=g) * 25
    return img.clamp(0, 255).to(torch.uint8)


def test_oracle_preprocess_shapes_and_identity():
    x = _frames((1, 224, 224), 1)[0]
    y = O.preprocess_image(x, 224)
    ref = (x.permute(2, 0, 1).float() / 255 - torch.tensor(O.OPENAI_DATASET_MEAN)[:, None, None]) / torch.tensor(O.OPENAI_DATASET_STD)[:, None, None]
    assert y.shape == (3, 224, 224) and torch.allclose(y, ref, atol=1e-5)      # same size: resize is the identity
    v = O.preprocess_video(_frames((4, 120, 200), 2), 56)
    assert v.shape == (3, 4, 56, 56)
    from vitron_amd.processing import sample_frame_indices
    assert sample_frame_indices(100, 8).tolist() == np.linspace(0, 99, 8, dtype=int).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,size", [((1, 480, 640), 224), ((1, 500, 333), 336), ((2, 224, 224), 224), ((1, 97, 131), 56)])
def test_image_preprocess_matches_oracle(shape, size):
    from vitron_amd.processing import LanguageBindImageProcessor, preprocess_frames
    dev = torch.device("cuda:0")
    fr = _frames(shape, 3)
    got = preprocess_frames(fr.to(dev), size, True, False, dtype=torch.float32).cpu()
    ref = torch.stack([O.preprocess_image(f, size) for f in fr])
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 2e-4          # fp32 tap weights in a different summation order
    proc = LanguageBindImageProcessor(image_size=size)
    pv = proc.preprocess([fr[0].numpy()], return_tensors="pt")["pixel_values"]
    assert pv.shape == (1, 3, size, size) and pv.dtype == torch.bfloat16 and proc.crop_size == {"height": size, "width": size}
    assert float((pv[0].float().cpu() - ref[0]).abs().max()) <= 2e-2   # bf16 output


@pytest.mark.gpu
@pytest.mark.parametrize("shape,size,flip", [((8, 360, 640), 224, False), ((8, 300, 200), 336, True), ((20, 64, 64), 56, False)])
def test_video_preprocess_matches_oracle(shape, size, flip):
    from vitron_amd.processing import LanguageBindVideoProcessor, preprocess_frames, sample_frame_indices
    dev = torch.device("cuda:0")
    fr = _frames(shape, 4)
    sel = fr[torch.from_numpy(sample_frame_indices(shape[0], 8))]
    got = preprocess_frames(sel.to(dev), size, False, True, flip=flip, dtype=torch.float32).cpu()
    ref = O.preprocess_video(sel, size, flip)
    assert got.shape == ref.shape == (3, 8, size, size)
    assert float((got - ref).abs().max()) <= 2e-4
    pv = LanguageBindVideoProcessor(image_size=size, num_frames=8, flip=flip)(fr)["pixel_values"]
    assert pv.shape == (1, 3, 8, size, size)
    assert float((pv[0].float().cpu() - ref).abs().max()) <= 2e-2


def test_oracle_preprocess_at_the_references_example_image_shapes_is_frozen():
    """tests/golden/preproc_shapes.json (make_golden_preproc.py): the oracle's restatement of the reference's image / video transforms on
    seeded pictures of the sizes of three of the reference's own COCO examples -- resized size, crop offsets, per-channel statistics,
    64 probe pixels, checksums. Pins the F.interpolate call, the size / crop arithmetic and the normalisation against drift; the size /
    crop RULES stay a restatement of torchvision / pytorchvideo (absent offline)."""
    import json
    import os

    from tests.golden import make_golden_preproc as mk
    with open(os.path.join(os.path.dirname(__file__), "golden", "preproc_shapes.json")) as f:
        gold = json.load(f)
    assert sorted({tuple(c["input_hw"]) for c in gold["cases"]}) == sorted(mk.EXAMPLE_HW) and len(gold["cases"]) == 6
    for c in gold["cases"]:
        x = mk.shapes_input(c["input_hw"], c["seed"])
        assert float(x.double().sum()) == c["in_checksum"], "the seeded inputs drifted from the fixture's"
        got = mk.describe(x, c["size"])
        assert got["input_hw"] == c["input_hw"] and got["resized_hw"] == c["resized_hw"] and got["crop_top_left"] == c["crop_top_left"]
        assert np.allclose(got["probe_values"], c["probe_values"], atol=2e-5) and np.allclose(got["video_probe_values"], c["video_probe_values"], atol=2e-5)
        assert abs(got["checksum"] - c["checksum"]) <= 1e-6 * c["checksum"] and abs(got["video_checksum"] - c["video_checksum"]) <= 1e-6 * c["video_checksum"]
        assert np.allclose(got["mean"], c["mean"], atol=1e-5) and np.allclose(got["std"], c["std"], atol=1e-5)


# ---- the reference's OWN processors (tests/golden/preproc_ref.npz; generator: make_golden_preproc.py::gen_ref) ------------------------
def _ref_cases():
    """(name, frames uint8 [F,H,W,3], flip or None for pictures, fixture entries) for every case of the fixture."""
    import os

    from tests.golden import cases
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "preproc_ref.npz"))
    inputs = cases.preproc_inputs()
    out = []
    for n in cases.PREPROC_IMAGES:
        assert float(inputs[n].double().sum()) == float(gold[n + "_in_checksum"]), "the seeded inputs drifted from the fixture's"
        out.append((n, inputs[n], None, gold[n + "_sub"], gold[n + "_sums"], None, cases.PREPROC_IMG_STRIDE))
    for n in cases.PREPROC_CLIPS:
        assert float(inputs[n].double().sum()) == float(gold[n + "_in_checksum"])
        for tag in ("keep", "flip"):
            if f"{n}_{tag}_sub" in gold.files:
                out.append((n, inputs[n], tag == "flip", gold[f"{n}_{tag}_sub"], gold[f"{n}_{tag}_sums"], gold[f"{n}_{tag}_idx"],
                            cases.PREPROC_CLIP_STRIDE))
    return out


def _against_fixture(y, sub, sums, stride, tol):
    y = y.float()
    assert float((y[..., ::stride, ::stride] - torch.from_numpy(sub)).abs().max()) <= tol
    yd = y.double().reshape(3, -1)
    got = torch.stack([yd.sum(1), yd.abs().sum(1), (yd * yd).sum(1)], 1).numpy()
    # (all pixels, not only the kept ones: sums of |.| and of squares within tol relative; the signed sum within tol per pixel)
    assert np.all(np.abs(got[:, 1:] - sums[:, 1:]) <= 2 * tol * sums[:, 1:] + 1e-9)
    assert np.all(np.abs(got[:, 0] - sums[:, 0]) <= tol * yd.shape[1])


def test_oracle_preprocess_matches_the_references_own_processors():
    """The oracle's restatement (and the product's frame sampling rule) against the reference's LanguageBindImageProcessor /
    LanguageBindVideoProcessor code, run unmodified over restated torchvision 0.15.2 / pytorchvideo 0.1.5 / decord / cv2 primitives
    (oracle/ref_preproc.py): transform order, the hard-wired 224, constants, x / 255, layout permutes, BGR -> RGB, the frames
    np.linspace picks (more, exactly, fewer frames than sampled), both outcomes of the inference-time random flip."""
    from vitron_amd.processing import sample_frame_indices
    seen_repeat = False
    for name, fr, flip, sub, sums, idx, stride in _ref_cases():
        if flip is None:
            y = O.preprocess_image(fr[0], 224)
        else:
            mine = sample_frame_indices(fr.shape[0], 8)
            assert mine.tolist() == idx.tolist(), name
            seen_repeat |= len(set(idx.tolist())) < 8
            y = O.preprocess_video(fr[torch.from_numpy(mine)], 224, flip)
        _against_fixture(y, sub, sums, stride, 2e-6)
    assert seen_repeat          # the fixture holds a clip with fewer frames than are sampled


@pytest.mark.gpu
def test_gpu_preprocess_matches_the_references_own_processors():
    """vt_preprocess through the product's processors (same entry points app.py uses) against the same fixture: fp32 output within 2e-4
    (fp32 tap weights in another summation order), 16-bit output within its rounding."""
    from vitron_amd.processing import LanguageBindImageProcessor, LanguageBindVideoProcessor
    ip = LanguageBindImageProcessor(image_size=224, dtype=torch.float32)
    for name, fr, flip, sub, sums, idx, stride in _ref_cases():
        if flip is None:
            y = ip.preprocess([fr[0].numpy()], return_tensors="pt")["pixel_values"][0]
            y16 = LanguageBindImageProcessor(image_size=224).preprocess([fr[0].numpy()], return_tensors="pt")["pixel_values"][0]
        else:
            y = LanguageBindVideoProcessor(image_size=224, num_frames=8, dtype=torch.float32, flip=flip)(fr)["pixel_values"][0]
            y16 = LanguageBindVideoProcessor(image_size=224, num_frames=8, flip=flip)(fr)["pixel_values"][0]
        assert y.dtype == torch.float32 and y16.dtype == torch.bfloat16
        _against_fixture(y.cpu(), sub, sums, stride, 2e-4)
        assert float((y16.float().cpu()[..., ::stride, ::stride] - torch.from_numpy(sub)).abs().max()) <= 2e-2
