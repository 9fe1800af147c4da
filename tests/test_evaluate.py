"""cabinet_amd.evaluate.MscEvalV0 on the CPU: the plain path against the reference's own evaluator (fixture g5_eval*.npz, written
by tests/golden/make_golden_eval.py from the imported reference), the histogram rules, the public contract, the two-rank reduce
and the C ABI declarations of the fused tail.

Near-ties: an argmax over fp32 sums cannot be demanded bit for bit.  A pixel is UNDECIDED when the reference's float64 top-two
margin is below TIE = 5 x ref32_vs_f64_maxabs (the distance between the reference's fp32 and float64 maps, read from the fixture).
Undecided pixels are at most 0.2 % of a case; every other pixel's prediction must equal the reference's, and the confusion
matrices must agree once the undecided pixels are removed from both (tests/eval_golden.py: check_against_case)."""
import os
import re
import socket

import numpy as np
import pytest
import torch

from eval_golden import CASES, StubNet, check_against_case, load_case, write_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _evaluator(g, model=None, **kw):
    from cabinet_amd.evaluate import MscEvalV0

    return MscEvalV0(model if model is not None else g["model"], [(g["image"], g["labels"])], g["n_classes"],
                     ignore_label=g["ignore_label"], scales=g["scales"], flip=g["flip"], cropsize=g["cropsize"], **kw)


_RECORD = {}


@pytest.mark.parametrize("case", CASES)
def test_plain_path_matches_the_reference(case):
    g = load_case(case)
    ev = _evaluator(g, fused=False)
    probs = ev.summed_probabilities(g["image"])
    assert probs.dtype == torch.float32 and tuple(probs.shape) == g["prob32"].shape
    res = ev.evaluate()
    check_against_case(g, probs, torch.argmax(probs, dim=1).numpy(), res, f"plain_cpu_case{case}", _RECORD)
    write_record(_RECORD, "plain_cpu")


@pytest.mark.parametrize("case", CASES)
def test_compute_hist_reproduces_the_fixture_matrix(case):
    """[pred, label] orientation, ignore_label dropped, every other label clipped into [0, C - 1]."""
    from cabinet_amd.evaluate import MscEvalV0

    g = load_case(case)
    C, lab = g["n_classes"], g["labels"].numpy()
    assert (lab == g["ignore_label"]).any() and ((lab >= C) & (lab != g["ignore_label"])).any()  # the fixture exercises both rules
    h = MscEvalV0.compute_hist(g["pred"][0], lab[0], C, g["ignore_label"])
    assert h.shape == (C, C) and np.array_equal(h, g["confusion_matrix"])
    assert np.array_equal(MscEvalV0.compute_hist(torch.from_numpy(g["pred"][0]), g["labels"][0], C, g["ignore_label"]), h)


def test_compute_hist_clips_and_orients():
    from cabinet_amd.evaluate import MscEvalV0

    pred = np.array([[0, 1, 2, 7], [3, 3, 0, 1]])
    label = np.array([[0, 2, 255, 200], [3, 9, 1, 255]])
    h = MscEvalV0.compute_hist(pred, label, 8, 255)
    want = np.zeros((8, 8), dtype=np.int64)
    for p, t in ((0, 0), (1, 2), (7, 7), (3, 3), (3, 7), (0, 1)):   # 200 and 9 count as class 7; the two 255s are dropped
        want[p, t] += 1
    assert np.array_equal(h, want)


def test_constructor_and_result_contract():
    import inspect

    from cabinet_amd.evaluate import MscEvalV0

    params = inspect.signature(MscEvalV0.__init__).parameters
    assert list(params) == ["self", "model", "dataloader", "n_classes", "ignore_label", "scales", "flip", "cropsize", "device", "fused"]
    assert [params[n].default for n in ("ignore_label", "scales", "flip", "cropsize", "device", "fused")] == [255, (1.0,), False, 1024, None, None]
    for name in ("pad_tensor", "eval_chip", "crop_eval", "scale_crop_eval", "compute_hist", "evaluate", "__call__"):
        assert callable(getattr(MscEvalV0, name))
    assert isinstance(inspect.getattr_static(MscEvalV0, "compute_hist"), staticmethod)
    g = load_case(4)
    ev = _evaluator(g)
    res = ev()
    assert set(res) == {"mIoU", "accuracy", "iou_per_class", "confusion_matrix"}
    C = g["n_classes"]
    assert list(res["iou_per_class"]) == [f"class_{i}" for i in range(C)]
    cm = res["confusion_matrix"]
    assert isinstance(cm, np.ndarray) and cm.dtype == np.float64 and cm.shape == (C, C)
    assert cm.sum() == float((g["labels"] != g["ignore_label"]).sum())
    diag = np.diag(cm)
    assert res["accuracy"] == diag.sum() / cm.sum()
    assert res["mIoU"] == np.nanmean(diag / (cm.sum(0) + cm.sum(1) - diag + 1e-8))
    # pad_tensor: centred zero padding and the indices of the original
    x = torch.arange(2 * 3 * 5 * 6, dtype=torch.float32).view(2, 3, 5, 6)
    padded, idx = ev.pad_tensor(x, (8, 11))
    assert idx == [1, 6, 2, 8] and tuple(padded.shape) == (2, 3, 8, 11)
    assert torch.equal(padded[:, :, 1:6, 2:8], x) and float(padded.sum()) == float(x.sum())


def test_labels_with_a_channel_axis():
    g = load_case(2)
    from cabinet_amd.evaluate import MscEvalV0

    kw = dict(ignore_label=g["ignore_label"], scales=g["scales"], flip=g["flip"], cropsize=g["cropsize"])
    a = MscEvalV0(g["model"], [(g["image"], g["labels"])], g["n_classes"], **kw).evaluate()
    b = MscEvalV0(g["model"], [(g["image"], g["labels"].unsqueeze(1))], g["n_classes"], **kw).evaluate()
    assert np.array_equal(a["confusion_matrix"], b["confusion_matrix"]) and a["mIoU"] == b["mIoU"]


def test_fused_on_a_cpu_model_raises_and_none_runs_plain():
    g = load_case(4)
    with pytest.raises(RuntimeError, match="not on a GPU"):
        _evaluator(g, fused=True).evaluate()
    auto, plain = _evaluator(g, fused=None).evaluate(), _evaluator(g, fused=False).evaluate()
    assert np.array_equal(auto["confusion_matrix"], plain["confusion_matrix"])


def _batches(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        lab = torch.randint(0, C, (2, 64, 96), generator=g)
        lab[torch.rand(2, 64, 96, generator=g) < 0.1] = 255
        out.append((torch.randn(2, 3, 64, 96, generator=g), lab))
    return out


def _stub(C, seed):
    torch.manual_seed(seed)
    net = StubNet(C)
    with torch.no_grad():
        net.conv.weight.mul_(4.0)
    return net.eval()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    import torch.distributed as dist

    from cabinet_amd.evaluate import MscEvalV0

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    batches = _batches(4, 8, seed=7)
    res = MscEvalV0(_stub(8, 3), batches[rank::world], 8, scales=(1.0, 0.75), flip=True, cropsize=48).evaluate()
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_rank_reduce_to_rank_zero(tmp_path):
    import torch.multiprocessing as mp

    from cabinet_amd.evaluate import MscEvalV0

    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r = [torch.load(tmp_path / f"r{i}.pt", weights_only=False) for i in range(world)]
    single = MscEvalV0(_stub(8, 3), _batches(4, 8, seed=7), 8, scales=(1.0, 0.75), flip=True, cropsize=48).evaluate()
    assert r[1] == {}
    assert np.array_equal(r[0]["confusion_matrix"], single["confusion_matrix"])
    assert r[0]["mIoU"] == single["mIoU"] and r[0]["accuracy"] == single["accuracy"]


def test_header_and_ctypes_table_list_the_eval_tail():
    from cabinet_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cabinet_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cabinet_[a-z0-9_]+)\s*\(", text))
    for name in ("cabinet_eval_chip_accum", "cabinet_eval_chip_accum_supported", "cabinet_eval_scale_merge", "cabinet_eval_argmax_hist"):
        assert name in declared and name in _lib.SIGNATURES
    assert "#define CABINET_ABI_VERSION 8" in text and _lib.ABI_VERSION == 8


def test_eval_tail_argument_errors_need_no_gpu():
    from cabinet_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.load()
    A = 0x10000
    assert lib.cabinet_eval_chip_accum_supported(19, 128, 128, 1024, 1024, 1) == 1      # the model's x8 output, config 5's crop
    assert lib.cabinet_eval_chip_accum_supported(19, 1024, 1024, 1024, 1024, 1) == 1    # a model without forward_lowres (factor 1)
    assert lib.cabinet_eval_chip_accum_supported(32, 13, 17, 100, 131, 1) == 1
    assert lib.cabinet_eval_chip_accum_supported(33, 16, 16, 128, 128, 0) == 0
    assert lib.cabinet_eval_chip_accum_supported(19, 128, 8192, 128, 128, 1) == 0       # x64 reduction: rows exceed the LDS
    rc = lib.cabinet_eval_chip_accum(A, None, 1, 8, 16, 16, 128, 128, A, 128, 200, 0, 73, None, None, None)
    assert rc == -1 and b"leaves" in lib.cabinet_last_error()                          # window past the right edge: never launched
    rc = lib.cabinet_eval_chip_accum(A, None, 1, 40, 16, 16, 128, 128, A, 128, 128, 0, 0, None, None, None)
    assert rc == -2 and b"max 32" in lib.cabinet_last_error()
    rc = lib.cabinet_eval_scale_merge(A, 1, 8, 128, 128, 10, 130, 0, 128, A, 64, 64, None)
    assert rc == -1 and b"leaves" in lib.cabinet_last_error()
    rc = lib.cabinet_eval_argmax_hist(A, A, 1, 33, 8, 8, 255, A, None, None)
    assert rc == -2
    rc = lib.cabinet_eval_argmax_hist(None, A, 1, 8, 8, 8, 255, A, None, None)
    assert rc == -1 and b"null" in lib.cabinet_last_error()
