"""Numpy restatement of msam2_label_confidence (csrc/volume_labels.hip) on a given array of up-sampled values v [T, n, H, W], and the count
fixtures its CPU and GPU tests share.  fp32 in: fp32 comparisons and ONE fp32 subtraction per voxel, as the kernel does them (the GPU test
feeds it ops.bilinear_upsample's output); float64 in (`volume_labels_restate.resize64`) for the dyadic fixtures, where both are exact.  The
margins and label_thr are rounded to fp32 first, as the device receives them, then compared in v's type.

Per voxel, one pass over the objects: tv = sv = -inf; v > tv: sv = tv, tv = v, to = o; else v > sv: sv = v (strict: ties to the lower index,
a tied value becomes sv, NaN never enters).  Labelled = tv > label_thr, m_in = tv - max(label_thr, sv); background with a finite tv: nearest
object `to`, m_out = label_thr - tv; a background voxel with no finite value is nobody's."""
import numpy as np

PROBABILITIES = (0.6, 0.75, 0.9)
EIGHT_MARGINS = (0.125, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 5.0)
DYADIC_MARGINS = (0.5, 1.0, 2.0)


def f32_margins(margins):
    return [float(np.float32(m)) for m in margins]


def logit_margins(ps):
    """log(p / (1 - p)) in float64, rounded to fp32: what volume_labels.margins_from_probabilities must return"""
    return [float(np.float32(np.log(np.float64(p) / (1.0 - np.float64(p))))) for p in ps]


def restate(v, ids, label_thr, margins, select):
    """v [T, n, H, W] float32 or float64 -> dict(labels, core, envelope, conf: uint8 [T, H, W]; counts: int64 [T, n, 2 + 2K]; to; m)"""
    v = np.asarray(v)
    assert v.dtype in (np.float32, np.float64)
    ft = v.dtype.type
    T, n, H, W = v.shape
    thr = ft(np.float32(label_thr))
    mg = [ft(m) for m in f32_margins(margins)]
    K = len(mg)
    tv = np.full((T, H, W), -np.inf, dtype=v.dtype)
    sv = np.full((T, H, W), -np.inf, dtype=v.dtype)
    to = np.full((T, H, W), -1, dtype=np.int64)
    for o in range(n):
        x = v[:, o]
        first = x > tv                                   # NaN compares false
        second = ~first & (x > sv)
        sv = np.where(first, tv, np.where(second, x, sv))
        tv = np.where(first, x, tv)
        to = np.where(first, o, to)
    lab = tv > thr
    near = ~lab & np.isfinite(tv)
    owned = lab | near
    with np.errstate(invalid="ignore"):
        m_in = (tv - np.maximum(thr, sv)).astype(v.dtype)
        m_out = (thr - tv).astype(v.dtype)
        m = np.where(lab, m_in, m_out)
        ge = np.stack([m >= g for g in mg])              # [K, T, H, W]
        lt = np.stack([m < g for g in mg])
    table = np.array(list(ids) + [0], dtype=np.uint8)    # index -1 = nobody
    id_to = table[np.where(owned, to, -1)]
    zero = np.zeros_like(id_to)
    labels = np.where(lab, id_to, zero)
    core = np.where(lab & ge[select], id_to, zero)
    envelope = np.where(lab | (near & lt[select]), id_to, zero)
    conf = np.where(owned, ge.sum(axis=0), K).astype(np.uint8)
    counts = np.zeros((T, n, 2 + 2 * K), dtype=np.int64)
    for o in range(n):
        mine = to == o
        counts[:, o, 0] = (mine & lab).sum(axis=(1, 2))
        counts[:, o, 1] = (v[:, o] > thr).sum(axis=(1, 2)) - counts[:, o, 0]
        for k in range(K):
            counts[:, o, 2 + k] = (mine & lab & lt[k]).sum(axis=(1, 2))
            counts[:, o, 2 + K + k] = (mine & near & lt[k]).sum(axis=(1, 2))
    return {"labels": labels, "core": core, "envelope": envelope, "conf": conf, "counts": counts, "to": to, "m": m, "lab": lab, "near": near}


def check_invariants(out, ids, margins, select, r):
    """What holds on every case, on the outputs `out` (dict of labels, core, envelope, conf, counts; any may be missing) of the code under test:
    core <= labels <= envelope per id; conf == K exactly where no band holds the voxel (a band holds it when an object owns it with
    m < margins[k]: the bands nest, so that is the widest one, taken from the restatement r's margins -- and, when select is the widest band,
    from the volumes themselves: labelled outside the core, or background inside the envelope); col 0 = the label histogram."""
    K = len(margins)
    has = lambda *names: all(out.get(k) is not None for k in names)                                        # noqa: E731
    for j, i in enumerate(ids):
        if has("core", "labels"):
            assert not ((out["core"] == i) & ~(out["labels"] == i)).any(), i
        if has("labels", "envelope"):
            assert not ((out["labels"] == i) & ~(out["envelope"] == i)).any(), i
        if has("labels", "counts"):
            assert np.array_equal(out["counts"][:, j, 0], (out["labels"] == i).sum(axis=(1, 2))), i
    if has("conf"):
        widest = (r["lab"] | r["near"]) & (r["m"] < r["m"].dtype.type(f32_margins(margins)[-1]))
        assert np.array_equal(out["conf"] == K, ~widest)
        assert out["conf"].max() <= K
        if select == K - 1 and has("labels", "core", "envelope"):
            lab = out["labels"] != 0
            assert np.array_equal(out["conf"] == K, ~np.where(lab, out["core"] == 0, out["envelope"] != 0))


def report_by_hand(counts, spacing=(1.0, 1.0, 1.0)):
    """confidence_report's integer figures from a count table, spelled out per organ and band with Python integers"""
    k = np.asarray(counts).astype(np.int64)
    T, n, cols = k.shape
    K = (cols - 2) // 2
    ml = float(spacing[0]) * float(spacing[1]) * float(spacing[2]) / 1000.0
    out = {"voxels": np.zeros(n, np.int64), "core_voxels": np.zeros((n, K), np.int64), "envelope_voxels": np.zeros((n, K), np.int64),
           "uncertain_fraction": np.full((n, K), np.nan), "overlap_voxels": np.zeros(n, np.int64)}
    for o in range(n):
        lab = sum(int(k[t, o, 0]) for t in range(T))
        out["voxels"][o] = lab
        out["overlap_voxels"][o] = sum(int(k[t, o, 1]) for t in range(T))
        for b in range(K):
            inside = sum(int(k[t, o, 2 + b]) for t in range(T))
            outside = sum(int(k[t, o, 2 + K + b]) for t in range(T))
            out["core_voxels"][o, b] = lab - inside
            out["envelope_voxels"][o, b] = lab + outside
            if lab + outside > 0:
                out["uncertain_fraction"][o, b] = (inside + outside) / (lab + outside)
    out["volume_ml"] = out["voxels"] * ml
    out["core_ml"] = out["core_voxels"] * ml
    out["envelope_ml"] = out["envelope_voxels"] * ml
    return out
