"""CPU checks of the prompt path (ops.label_stats / ops.label_pick / prompts.py): the numpy restatement the GPU test compares with is what
the dataset's data.generate_bbox and data.random_click compute, pair by pair; the u -> k rule is Python integer arithmetic; the entries'
limits and the wrappers' checks act before anything touches a device."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prompts_restate as R  # noqa: E402

SMALL = [(name, vol, ids) for name, vol, ids in R.cases() if vol.size <= 9 * 130 * 100]


@pytest.mark.parametrize("name,vol,ids", SMALL, ids=[c[0] for c in SMALL])
@pytest.mark.parametrize("seed", [0, 7])
def test_restatement_is_what_the_dataset_computes(name, vol, ids, seed):
    import medical_sam2_amd.data as data
    st, rows = R.stats(vol, ids)
    count = st[..., 0]
    k = np.zeros_like(count)
    for d, j in zip(*np.nonzero(count)):
        k[d, j] = random.Random(seed).randint(0, int(count[d, j]) - 1)        # data.random_click's draw
    xy = R.pick(vol, ids, k)
    for d in range(vol.shape[0]):
        for j, v in enumerate(ids):
            mask = (vol[d] == v).astype(np.uint8)
            box = data.generate_bbox(mask)
            if count[d, j] == 0:
                assert np.isnan(box).all() and st[d, j].tolist() == [0, -1, -1, -1, -1] and xy[d, j].tolist() == [-1, -1]
                continue
            assert box.tolist() == [st[d, j, 3], st[d, j, 1], st[d, j, 4], st[d, j, 2]]
            label, click = data.random_click(mask, 1, seed=seed)
            assert label == 1 and click.tolist() == xy[d, j].tolist()
            assert rows[d, j].tolist() == mask.sum(axis=1).tolist() and count[d, j] == mask.sum()


def test_fixtures_do_what_they_are_for():
    seen = {name: (vol, ids) for name, vol, ids in R.cases()}
    assert len(seen) >= 30 and {tuple(v.shape) for v, _ in seen.values()} == set(R.SHAPES)
    for name, (vol, ids) in seen.items():
        assert vol.dtype == np.uint8 and 1 <= len(ids) <= 32 and len(set(ids)) == len(ids) and all(1 <= v <= 255 for v in ids), name
    st = {name: R.stats(*seen[name])[0] for name in ("blobs32_9x130x100", "full_3x64x64", "corners_3x64x64", "lines_3x64x64")}
    c = st["blobs32_9x130x100"][..., 0]
    assert (c == 0).any() and (c > 0).any()                                   # an object absent on some slices
    assert st["full_3x64x64"][0, 0].tolist() == [64 * 64, 0, 63, 0, 63] and st["full_3x64x64"][0, 1, 0] == 0
    assert (st["corners_3x64x64"][..., 0] == 1).all()
    assert st["lines_3x64x64"][0, 0].tolist() == [63, 0, 62, 21, 21] and st["lines_3x64x64"][0, 1].tolist() == [63, 32, 32, 0, 63]
    assert st["blobs32_9x130x100"].shape[1] == 32
    vol, ids = seen["checkerboard_3x64x64"]
    assert set(np.unique(vol)) - set(ids) == {77}                             # a value in the volume that is nobody's id
    vol, ids = seen["blobs13_1x1024x1024b"]
    assert set(np.unique(vol)) - set(ids) - {0}


def test_u_to_k_is_integer_arithmetic_and_stays_in_range():
    rng = np.random.RandomState(0)
    count = np.concatenate([[1, 1, 2, 3, 8192 * 8192, 8192 * 8192, 8192 * 8192], rng.randint(1, 8192 * 8192 + 1, 2000)])
    u = np.concatenate([[0, 2 ** 32 - 1, 2 ** 31, 2 ** 32 - 1, 0, 2 ** 32 - 1, 2 ** 32 - 2], rng.randint(0, 2 ** 32, 2000, dtype=np.int64)])
    k = R.k_from_u(u, count)
    assert k.tolist() == [(int(a) * int(b)) >> 32 for a, b in zip(u, count)]
    assert (k >= 0).all() and (k < count).all()
    assert R.k_from_u(2 ** 32 - 1, 5) == 4 and R.k_from_u(0, 5) == 0


def test_argument_errors_cross_the_abi_as_codes():
    """the limits of msam2_label_stats / msam2_label_pick are refused on the host, before the device is touched, naming the entry"""
    from medical_sam2_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    ptr = (ctypes.addressof(buf) + 15) & ~15                 # a valid host address: never dereferenced by the checks
    ok = dict(labels=ptr, ids=ptr, D=1, H=8, W=8, n=2, stats=ptr, rows=ptr, k=ptr, u=None, xy=ptr)
    entries = {
        "label_stats": lambda a: L.msam2_label_stats(a["labels"], a["ids"], a["D"], a["H"], a["W"], a["n"], a["stats"], a["rows"], None),
        "label_pick": lambda a: L.msam2_label_pick(a["labels"], a["ids"], a["stats"], a["rows"], a["k"], a["u"], a["D"], a["H"], a["W"], a["n"],
                                                   a["xy"], None),
    }
    shared = {"n = 0": dict(n=0), "n = 33": dict(n=33), "D 0 ": dict(D=0), "D 65536": dict(D=65536), "0x8": dict(H=0), "8193x8": dict(H=8193),
              "8x0": dict(W=0), "8x8193": dict(W=8193), "null": dict(labels=None), "null ": dict(ids=None), " null": dict(stats=None),
              "null labels": dict(rows=None)}
    for entry, call in entries.items():
        own = dict(shared, **({"exactly one": dict(k=None), "exactly one ": dict(u=ptr), "null  ": dict(xy=None)} if entry == "label_pick" else {}))
        for what, kw in own.items():
            rc = call(dict(ok, **kw))
            msg = L.msam2_last_error().decode()
            assert rc < 0, (entry, what, rc)
            assert msg.startswith(entry + ":") and what.strip() in msg, (entry, what, msg)


def test_ops_refuse_bad_arguments():
    import medical_sam2_amd.ops as ops
    vol = torch.zeros(2, 8, 8, dtype=torch.uint8)
    stats, rows = torch.zeros(2, 2, 5, dtype=torch.int32), torch.zeros(2, 2, 8, dtype=torch.int32)
    k = torch.zeros(2, 2, dtype=torch.int32)
    for what, call in {
        "uint8": lambda: ops.label_stats(vol.int(), [1, 2]),
        "uint8 ": lambda: ops.label_stats(vol.float(), [1, 2]),
        "contiguous": lambda: ops.label_stats(vol.transpose(1, 2), [1, 2]),
        "contiguous ": lambda: ops.label_stats(vol[:, :, ::2], [1, 2]),
        r"\[D, H, W\]": lambda: ops.label_stats(vol[0], [1, 2]),
        "distinct": lambda: ops.label_stats(vol, [4, 4]),
        "1 .. 255": lambda: ops.label_stats(vol, [0, 1]),
        "1 .. 32": lambda: ops.label_stats(vol, list(range(1, 34))),
        "1 .. 32 ": lambda: ops.label_pick(vol, list(range(1, 34)), stats, rows, k=k),
        "uint8  ": lambda: ops.label_pick(vol.int(), [1, 2], stats, rows, k=k),
        "on the GPU": lambda: ops.label_stats(vol, [1, 2]),
    }.items():
        with pytest.raises(ValueError, match=what.strip()):
            call()
    assert ops.LABEL_MAX_OBJECTS == 32


def test_prompts_module_refuses_before_the_device():
    from medical_sam2_amd import prompts
    vol = torch.zeros(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="Prompt not recognized"):
        prompts.label_prompts(vol, [1], prompt="mask")
    with pytest.raises(AssertionError, match="uint8"):
        prompts.label_prompts(vol.float(), [1])
    t = prompts.targets_from_labels(torch.tensor([[[0, 3], [250, 3]]], dtype=torch.uint8), [3, 250])
    assert sorted(t) == [0] and t[0].shape == (2, 1, 2, 2) and t[0].dtype == torch.float32
    assert t[0][:, 0].tolist() == [[[0, 1], [0, 1]], [[0, 0], [1, 0]]]
    box = prompts._jitter(2, 9, 4, 30, 0, None)
    assert box.tolist() == [4, 2, 30, 9] and box.dtype == np.int64
