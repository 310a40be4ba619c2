"""Label confidence without a GPU: every refusal of msam2_label_confidence through the C ABI with fake pointers (a refused call launches
nothing), return code and full text; the host halves (volume_labels.margins_from_probabilities, confidence_report, prompts.review_slices) on
hand-made count tables; and the facts about the shared fixtures that keep tests/test_label_confidence_gpu.py from being vacuous, recomputed
here with the float64 resize of tests/volume_labels_restate.py."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import confidence_restate as C  # noqa: E402
import volume_labels_restate as R  # noqa: E402

MSAM2_ERR_ARG = -1
NAN, INF = float("nan"), float("inf")


def _call(n=2, T=2, lh=4, lw=4, H=8, W=8, margins=(0.5, 1.0, 2.0), K=None, select=1, logits=True, ids=True, null_margins=False, outputs=(1, 1, 1, 1, 1)):
    from medical_sam2_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    m = (ctypes.c_float * max(len(margins), 1))(*margins)
    K = len(margins) if K is None else K
    outs = [ptr if o else None for o in outputs]
    rc = L.msam2_label_confidence(ptr if logits else None, ptr if ids else None, T, n, lh, lw, H, W, 0.0, None if null_margins else m, K, select, *outs, None)
    return rc, L.msam2_last_error().decode()


CASES = [
    (dict(logits=False), 'label_confidence: null logits / ids / margins'),
    (dict(ids=False), 'label_confidence: null logits / ids / margins'),
    (dict(null_margins=True), 'label_confidence: null logits / ids / margins'),
    (dict(n=0), 'label_confidence: n = 0 objects (1 .. 32 per call)'),
    (dict(n=33), 'label_confidence: n = 33 objects (1 .. 32 per call)'),
    (dict(K=0), 'label_confidence: K = 0 margins (1 .. 8 per call)'),
    (dict(K=9), 'label_confidence: K = 9 margins (1 .. 8 per call)'),
    (dict(K=-1), 'label_confidence: K = -1 margins (1 .. 8 per call)'),
    (dict(T=0), 'label_confidence: bad sizes (T 0, low-res 4x4, output 8x8)'),
    (dict(T=65536), 'label_confidence: bad sizes (T 65536, low-res 4x4, output 8x8)'),
    (dict(H=0), 'label_confidence: bad sizes (T 2, low-res 4x4, output 0x8)'),
    (dict(W=0), 'label_confidence: bad sizes (T 2, low-res 4x4, output 8x0)'),
    (dict(lh=0), 'label_confidence: bad sizes (T 2, low-res 0x4, output 8x8)'),
    (dict(lw=0), 'label_confidence: bad sizes (T 2, low-res 4x0, output 8x8)'),
    (dict(H=65536, W=32768), 'label_confidence: bad sizes (T 2, low-res 4x4, output 65536x32768)'),
    (dict(lh=65536, lw=32768), 'label_confidence: bad sizes (T 2, low-res 65536x32768, output 8x8)'),
    (dict(margins=(0.0, 1.0)), 'label_confidence: margins[0] = 0 (finite, positive and strictly ascending)'),
    (dict(margins=(-0.5, 1.0)), 'label_confidence: margins[0] = -0.5 (finite, positive and strictly ascending)'),
    (dict(margins=(NAN, 1.0)), 'label_confidence: margins[0] = nan (finite, positive and strictly ascending)'),
    (dict(margins=(0.5, INF)), 'label_confidence: margins[1] = inf (finite, positive and strictly ascending)'),
    (dict(margins=(0.5, 0.5, 2.0)), 'label_confidence: margins[1] = 0.5 (finite, positive and strictly ascending)'),
    (dict(margins=(0.5, 1.0, 0.75)), 'label_confidence: margins[2] = 0.75 (finite, positive and strictly ascending)'),
    (dict(margins=(0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 5.5)), 'label_confidence: margins[7] = 5.5 (finite, positive and strictly ascending)'),
    (dict(select=-1), 'label_confidence: select = -1 (0 .. 2)'),
    (dict(select=3), 'label_confidence: select = 3 (0 .. 2)'),
    (dict(margins=(0.5,), select=1), 'label_confidence: select = 1 (0 .. 0)'),
    (dict(outputs=(0, 0, 0, 0, 0)), 'label_confidence: no output requested (labels, core, envelope, conf, counts)'),
]


@pytest.mark.parametrize("bad, text", CASES, ids=["%s" % ", ".join("%s=%r" % kv for kv in b.items()) for b, _ in CASES])
def test_refusal_code_and_text(bad, text):
    rc, msg = _call(**bad)
    assert rc == MSAM2_ERR_ARG, (rc, msg)
    assert msg == text


def test_refusals_come_in_the_documented_order():
    """null pointers, objects, K, sizes, margins, select, outputs: the first that fails is the one reported"""
    assert _call(n=0, K=0)[1] == 'label_confidence: n = 0 objects (1 .. 32 per call)'
    assert _call(K=9, T=0)[1] == 'label_confidence: K = 9 margins (1 .. 8 per call)'
    assert _call(T=0, margins=(0.0,), select=0)[1] == 'label_confidence: bad sizes (T 0, low-res 4x4, output 8x8)'
    assert _call(margins=(1.0, 0.5), select=5)[1] == 'label_confidence: margins[1] = 0.5 (finite, positive and strictly ascending)'
    assert _call(select=5, outputs=(0, 0, 0, 0, 0))[1] == 'label_confidence: select = 5 (0 .. 2)'


def test_wrapper_refusals_keep_their_text():
    import medical_sam2_amd.ops as ops
    logits = torch.zeros(2, 2, 4, 4)
    cases = [
        (lambda: ops.label_confidence(logits.double(), [1, 2], 8, 8, (0.5,)), "label_confidence: fp32 contiguous [T, n, lh, lw]"),
        (lambda: ops.label_confidence(logits[:, :, :, ::2], [1, 2], 8, 8, (0.5,)), "label_confidence: fp32 contiguous [T, n, lh, lw]"),
        (lambda: ops.label_confidence(logits, [1, 2, 3], 8, 8, (0.5,)), "label_confidence: 2 objects need 2 uint8 ids"),
        (lambda: ops.label_confidence(logits, [4, 4], 8, 8, (0.5,)), "label_slices: ids must be distinct"),
        (lambda: ops.label_confidence(logits, [1, 2], 8, 8, (0.5,), core=torch.zeros(2, 8, 8, dtype=torch.int8)),
         "label_confidence: core must be uint8 contiguous [2, 8, 8] on the logits' device"),
        (lambda: ops.label_confidence(logits, [1, 2], 8, 8, (0.5,), conf=torch.zeros(2, 8, 9, dtype=torch.uint8)),
         "label_confidence: conf must be uint8 contiguous [2, 8, 8] on the logits' device"),
        (lambda: ops.label_confidence(logits, [1, 2], 8, 8, (0.5, 1.0), counts=torch.zeros(2, 2, 4, dtype=torch.int32)),
         "label_confidence: counts must be int32 contiguous [2, 2, 6] on the logits' device"),
        (lambda: ops.label_confidence(logits, [1, 2], 8, 8, (0.5, 1.0), counts=torch.zeros(2, 2, 6, dtype=torch.int64)),
         "label_confidence: counts must be int32 contiguous [2, 2, 6] on the logits' device"),
    ]
    for call, text in cases:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text


def test_margins_from_probabilities():
    from medical_sam2_amd.volume_labels import margins_from_probabilities
    m = margins_from_probabilities((0.6, 0.75, 0.9))
    assert list(m) == C.logit_margins((0.6, 0.75, 0.9)) and isinstance(m, tuple)
    assert all(float(np.float32(v)) == v for v in m) and m[0] < m[1] < m[2]                 # fp32 values, ascending with p
    assert m[1] == float(np.float32(math.log(3.0)))
    assert abs(1.0 / (1.0 + math.exp(-m[2])) - 0.9) < 1e-7                                  # a margin is the logit of its probability
    for bad in (0.5, 1.0, 0.3, 1.5, NAN):
        with pytest.raises(ValueError, match="winning probability"):
            margins_from_probabilities((0.6, bad))


# counts [T = 3, n = 3, 2 + 2K] with K = 2: (label, overlap, inside_0, inside_1, outside_0, outside_1)
TABLE = np.array([[[100, 7, 10, 30, 5, 20], [0, 0, 0, 0, 0, 0], [50, 0, 0, 50, 0, 9]],
                  [[200, 0, 20, 40, 0, 10], [0, 3, 0, 0, 0, 0], [50, 1, 0, 50, 0, 9]],
                  [[0, 0, 0, 0, 4, 8], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]]], dtype=np.int32)


def test_confidence_report_on_a_hand_made_table():
    from medical_sam2_amd.volume_labels import confidence_report
    sp = (2.5, 0.8, 0.8)
    rep = confidence_report(TABLE, spacing=sp)
    hand = C.report_by_hand(TABLE, sp)
    for key, want in hand.items():
        assert np.array_equal(rep[key], want, equal_nan=True), key
    # spelled out: organ 0 holds 300 voxels; band 1 takes 70 of them out of the core and adds 38 background voxels to the envelope
    assert rep["voxels"].tolist() == [300, 0, 100] and rep["overlap_voxels"].tolist() == [7, 3, 1]
    assert rep["core_voxels"].tolist() == [[270, 230], [0, 0], [100, 0]]
    assert rep["envelope_voxels"].tolist() == [[309, 338], [0, 0], [100, 118]]
    assert rep["uncertain_voxels"].tolist() == [[39, 108], [0, 0], [0, 118]]
    assert rep["uncertain_fraction"][0].tolist() == [39 / 309, 108 / 338] and rep["uncertain_fraction"][2].tolist() == [0.0, 1.0]
    assert np.isnan(rep["uncertain_fraction"][1]).all()                                      # an empty envelope: NaN, not 0
    ml = 2.5 * 0.8 * 0.8 / 1000.0
    assert rep["volume_ml"].tolist() == [300 * ml, 0.0, 100 * ml] and rep["core_ml"][0].tolist() == [270 * ml, 230 * ml]
    assert rep["envelope_ml"][2].tolist() == [100 * ml, 118 * ml]
    # per slice: the same figures with a leading slice axis; slice 2 has an envelope without a label
    per = rep["per_slice"]
    assert per["voxels"].shape == (3, 3) and per["core_voxels"].shape == (3, 3, 2) and per["uncertain_fraction"].shape == (3, 3, 2)
    for t in range(3):
        one = C.report_by_hand(TABLE[t: t + 1], sp)
        for key, want in one.items():
            assert np.array_equal(per[key][t], want, equal_nan=True), (t, key)
    assert per["uncertain_fraction"][2, 0].tolist() == [1.0, 1.0] and np.isnan(per["uncertain_fraction"][2, 1:]).all()
    assert "slice_dice" not in rep
    # adjacent-slice Dice from int64 sums; both slices empty: NaN; one empty: 0
    cons = np.array([[[90, 100, 200], [0, 0, 0], [50, 50, 50]], [[0, 200, 0], [0, 0, 0], [0, 50, 0]]], dtype=np.int32)
    rep = confidence_report(TABLE, cons, sp)
    assert rep["slice_dice"].shape == (2, 3)
    assert rep["slice_dice"][0].tolist()[::2] == [180 / 300, 1.0] and rep["slice_dice"][1].tolist()[::2] == [0.0, 0.0]
    assert np.isnan(rep["slice_dice"][:, 1]).all()
    big = np.array([[[2 ** 31 - 1, 0, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1]]] * 4, dtype=np.int32)   # sums past int32
    rep = confidence_report(big)
    assert rep["envelope_voxels"].tolist() == [[8 * (2 ** 31 - 1)] * 2] and rep["core_voxels"].tolist() == [[0, 0]]
    assert rep["uncertain_fraction"].tolist() == [[1.0, 1.0]]
    # tensors take the same road (on the CPU: the copy is a no-op)
    rep_t = confidence_report(torch.from_numpy(TABLE), torch.from_numpy(cons), sp)
    assert np.array_equal(rep_t["envelope_voxels"], confidence_report(TABLE, cons, sp)["envelope_voxels"]) and rep_t["slice_dice"].shape == (2, 3)


def test_review_slices_on_a_hand_made_table():
    from medical_sam2_amd.prompts import review_slices, worst_slices
    counts = torch.from_numpy(TABLE)
    # band 1: uncertain = inside_1 + outside_1 = object 0: (50, 50, 8), object 1: none, object 2: (59, 59, 0)
    assert review_slices(counts, 1, 1).tolist() == [[0], [-1], [0]]                          # ties go to the lower slice
    assert review_slices(counts, 1, 3).tolist() == [[0, 1, 2], [-1, -1, -1], [0, 1, -1]]     # fewer than per_object uncertain slices: -1
    assert review_slices(counts, 1, 5).tolist() == [[0, 1, 2, -1, -1], [-1] * 5, [0, 1, -1, -1, -1]]   # more than there are slices
    # band 0: object 0: (15, 20, 4), object 2: nothing
    assert review_slices(counts, 0, 2).tolist() == [[1, 0], [-1, -1], [-1, -1]]
    both = torch.stack([counts[..., 3], counts[..., 5]], dim=-1)
    assert torch.equal(review_slices(counts, 1, 2), worst_slices(both, 2)) and review_slices(counts, 1, 2).dtype == torch.int64
    for band in (-1, 2):
        with pytest.raises(AssertionError, match="band"):
            review_slices(counts, band)
    with pytest.raises(AssertionError, match="counts"):
        review_slices(counts[..., :5], 0)


def test_restatement_on_a_voxel_table():
    """the rule on six hand-made voxels, two objects, label_thr 0.25, margins (0.5, 1): each line of the definitions once"""
    v = np.array([[3.0, 1.0],          # labelled 0, m = 3 - max(0.25, 1) = 2: beyond both bands
                  [1.0, 1.0],          # a tie: the lower index wins, the tied value is sv, m = 0
                  [0.5, NAN],          # NaN never enters: labelled 0 against the threshold, m = 0.25
                  [0.25, -2.0],        # exactly at the threshold: background, nearest 0, m_out = 0
                  [-1.0, -0.5],        # background, nearest 1, m_out = 0.75: in band 1 only
                  [NAN, -INF]],        # no finite value: nobody's
                 dtype=np.float32).T.reshape(1, 2, 1, 6)
    for vv in (v, v.astype(np.float64)):
        r = C.restate(vv, [7, 9], 0.25, (0.5, 1.0), 1)
        assert r["labels"].tolist() == [[[7, 7, 7, 0, 0, 0]]]
        assert r["core"].tolist() == [[[7, 0, 0, 0, 0, 0]]]
        assert r["envelope"].tolist() == [[[7, 7, 7, 7, 9, 0]]]
        assert r["conf"].tolist() == [[[2, 0, 0, 0, 1, 2]]]
        assert r["counts"].tolist() == [[[3, 0, 2, 2, 1, 1], [0, 2, 0, 0, 0, 1]]]            # object 1 is above 0.25 twice, and 0 took both voxels
        C.check_invariants(r, [7, 9], (0.5, 1.0), 1, r)
        r0 = C.restate(vv, [7, 9], 0.25, (0.5, 1.0), 0)
        assert r0["core"].tolist() == [[[7, 0, 0, 0, 0, 0]]] and r0["envelope"].tolist() == [[[7, 7, 7, 7, 0, 0]]]
        assert np.array_equal(r0["counts"], r["counts"]) and np.array_equal(r0["conf"], r["conf"])


NON_VACUOUS = {0: 47, 6: 374}          # index into R.SHAPES -> the smallest per-object column sum over both thresholds


@pytest.mark.parametrize("index", sorted(NON_VACUOUS))
def test_fixture_facts_every_column_of_every_object_is_hit(index):
    """On the 3 x 3 (16^2 -> 37 x 53) and 1 x 4 (64^2 -> 256^2) fixtures every object has a non-zero sum in every column, at label_thr 0 and
    1.5, with the margins of (0.6, 0.75, 0.9): the equality the GPU test asserts there is about numbers, not about zeros.  Float64 resize."""
    T, n, (lh, lw), (H, W) = R.SHAPES[index]
    smallest = None
    for seed in R.SEEDS:
        v = R.resize64(R.random_logits(T, n, lh, lw, seed).numpy(), H, W)
        for thr in (0.0, 1.5):
            r = C.restate(v, R.random_ids(n, seed), thr, C.logit_margins(C.PROBABILITIES), 1)
            per_object = r["counts"].sum(axis=0)                                            # [n, 2 + 2K]
            assert (per_object > 0).all(), (seed, thr, per_object)
            assert 0 in r["labels"] and (r["core"] != r["labels"]).any() and (r["envelope"] != r["labels"]).any()
            assert len(np.unique(r["conf"])) == 4
            smallest = int(per_object.min()) if smallest is None else min(smallest, int(per_object.min()))
    print("smallest per-object column sum:", smallest)
    assert smallest == NON_VACUOUS[index]


def test_fixture_facts_dyadic_ties_and_threshold_hits():
    """the dyadic fixtures hold margin 0 (ties between the repeated planes) and values exactly at a threshold, at both thresholds of the GPU test"""
    for (lh, lw), (H, W) in R.DYADIC_CASES:
        v = R.resize64(R.dyadic_logits(2, lh, lw, seed=H).numpy(), H, W)
        assert v.dtype == np.float64 and np.array_equal(v, v.astype(np.float32).astype(np.float64))          # exact in fp32 too
        for thr in (0.0, 1.25):
            r = C.restate(v, R.random_ids(6, seed=H), thr, C.DYADIC_MARGINS, 1)
            assert ((r["m"] == 0) & r["lab"]).sum() > 0 and ((r["m"] == 0) & r["near"]).sum() > (0 if thr else 10)
            assert any((r["m"] == g).any() for g in C.DYADIC_MARGINS)                                        # a margin exactly on a band edge
            assert (r["counts"].sum(axis=(0, 1)) > 0).all()
