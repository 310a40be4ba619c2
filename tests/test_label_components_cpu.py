"""Connected components / island removal / overlap counts of label volumes, the part that needs no GPU: the restatement the GPU tests compare
against (tests/components_restate.py) is itself checked against an independent flood fill and hand-written cases, the new entries refuse bad
arguments across the C ABI with a code (host pointers that are never dereferenced, as tests/test_abi.py does), and the wrappers check theirs."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import components_restate as R  # noqa: E402


def _tiny_volumes():
    rng = np.random.RandomState(0)
    yield "noise3", rng.randint(0, 3, (6, 7, 9)).astype(np.uint8)
    yield "noise2_dense", (rng.rand(5, 7, 9) < 0.7).astype(np.uint8)
    yield "sparse", (rng.rand(6, 7, 9) < 0.2).astype(np.uint8) * 9
    yield "parity", R.parity_lattice((4, 6, 8))
    yield "diagonal", R.diagonal_lattice((5, 7, 9)) * 200
    yield "serpentine", R.serpentine((3, 7, 6))
    yield "one_voxel", np.ones((1, 1, 1), dtype=np.uint8)
    yield "full", np.full((2, 3, 4), 7, dtype=np.uint8)


@pytest.mark.parametrize("name,vol", list(_tiny_volumes()), ids=[n for n, _ in _tiny_volumes()])
def test_restatement_equals_a_flood_fill(name, vol):
    for conn in R.CONNECTIVITIES:
        comp, size = R.restate(vol, conn)
        f_comp, f_size = R.flood(vol, conn)
        assert np.array_equal(comp, f_comp) and np.array_equal(size, f_size), conn
        assert (comp > 0).sum() == (vol > 0).sum() == size.sum()
        heads = np.flatnonzero(size.reshape(-1) > 0)
        assert np.array_equal(comp.reshape(-1)[heads], heads + 1)


def test_fixtures_tell_the_connectivities_apart():
    vol = R.parity_lattice((4, 6, 8))
    assert [R.n_components(R.restate(vol, c)[1]) for c in (4, 8, 6, 18, 26)] == [96, 4, 96, 1, 1]
    lat = R.diagonal_lattice((5, 7, 9))
    assert R.n_components(R.restate(lat, 18)[1]) == int(lat.sum()) and R.n_components(R.restate(lat, 26)[1]) == 1
    snake = R.serpentine((5, 9, 6))
    assert [R.n_components(R.restate(snake, c)[1]) for c in (4, 8, 6, 18, 26)] == [5, 5, 1, 1, 1]


def test_clean_rules_on_hand_written_cases():
    # value 3: components of 2, 2 (a tie: the earlier one is the largest) and 1 voxels; value 5: one component of 3 voxels; value 8: not listed
    vol = np.array([[[3, 3, 0, 3, 3, 0, 3],
                     [0, 0, 0, 0, 0, 0, 0],
                     [5, 5, 5, 0, 8, 8, 0]]], dtype=np.uint8)
    comp, size = R.restate(vol, 6)
    assert size[0, 0].tolist() == [2, 0, 0, 2, 0, 0, 1] and comp[0, 0].tolist() == [1, 1, 0, 4, 4, 0, 7]
    out, info = R.clean(vol, comp, size, [5, 3], None, 0b10)                       # ids in non-ascending order; largest of value 3 only
    assert out[0, 0].tolist() == [3, 3, 0, 0, 0, 0, 0] and out[0, 2].tolist() == [5, 5, 5, 0, 8, 8, 0]
    assert info.tolist() == [[1, 3, 3, 15, 1, 3], [3, 5, 2, 1, 1, 2]]
    out, info = R.clean(vol, comp, size, [5, 3], [0, 2], 0)                        # a voxel count alone
    assert out[0, 0].tolist() == [3, 3, 0, 3, 3, 0, 0] and info[1].tolist() == [3, 5, 2, 1, 2, 4]
    out, info = R.clean(vol, comp, size, [5, 3], [4, 3], 0b11)                     # the largest is below min_voxels: the organ vanishes
    assert not out[0, 0].any() and not out[0, 2, :3].any() and out[0, 2, 4:6].tolist() == [8, 8]
    assert info.tolist() == [[1, 3, 3, 15, 0, 0], [3, 5, 2, 1, 0, 0]]
    out, info = R.clean(vol, comp, size, [9], None, 1)                             # an absent value
    assert np.array_equal(out, vol) and info.tolist() == [[0, 0, 0, 0, 0, 0]]
    assert R.overlap(vol, out, [3, 5, 9]).tolist() == [[[5, 5, 5], [3, 3, 3], [0, 0, 0]]]


def test_argument_errors_cross_the_abi_as_codes():
    from medical_sam2_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    big = 1 << 40
    assert L.msam2_label_components_workspace_bytes(2, 3, 5) == 2 * 3 * 5 * 4 and L.msam2_label_components_workspace_bytes(1, 1, 8193) == 0
    assert L.msam2_label_clean_workspace_bytes(0) == 0 and L.msam2_label_clean_workspace_bytes(33) == 0
    assert 0 < L.msam2_label_clean_workspace_bytes(1) <= 4096 and L.msam2_label_clean_workspace_bytes(32) <= 4096
    cases = {
        "label_components: connectivity 7": lambda: L.msam2_label_components(ptr, 2, 4, 4, 7, ptr, ptr, ptr, big, None),
        "label_components: connectivity 0": lambda: L.msam2_label_components(ptr, 2, 4, 4, 0, ptr, ptr, ptr, big, None),
        "label_components: voxels": lambda: L.msam2_label_components(ptr, 33, 8192, 8192, 26, ptr, ptr, ptr, big, None),      # 2^31 + 2^26 voxels
        "label_components: 2^31 - 1": lambda: L.msam2_label_components(ptr, 1, 1, 2 ** 31 - 1, 26, ptr, ptr, ptr, big, None),
        "label_components: W": lambda: L.msam2_label_components(ptr, 1, 4, 8193, 26, ptr, ptr, ptr, big, None),
        "label_components: D": lambda: L.msam2_label_components(ptr, 65536, 4, 4, 26, ptr, ptr, ptr, big, None),
        "label_components: H": lambda: L.msam2_label_components(ptr, 1, 0, 4, 26, ptr, ptr, ptr, big, None),
        "label_components: workspace": lambda: L.msam2_label_components(ptr, 2, 4, 4, 26, ptr, ptr, ptr, 2 * 4 * 4 * 4 - 1, None),
        "label_components: null comp": lambda: L.msam2_label_components(ptr, 2, 4, 4, 26, None, ptr, ptr, big, None),
        "label_components: null size": lambda: L.msam2_label_components(ptr, 2, 4, 4, 26, ptr, None, ptr, big, None),
        "label_components: null labels": lambda: L.msam2_label_components(None, 2, 4, 4, 26, ptr, ptr, ptr, big, None),
        "label_components: null workspace": lambda: L.msam2_label_components(ptr, 2, 4, 4, 26, ptr, ptr, None, big, None),
        "label_clean: n = 0": lambda: L.msam2_label_clean(ptr, ptr, ptr, ptr, 0, None, 0, ptr, ptr, ptr, big, 2, 4, 4, None),
        "label_clean: n = 33": lambda: L.msam2_label_clean(ptr, ptr, ptr, ptr, 33, None, 0, ptr, ptr, ptr, big, 2, 4, 4, None),
        "label_clean: workspace": lambda: L.msam2_label_clean(ptr, ptr, ptr, ptr, 4, None, 0, ptr, ptr, ptr,
                                                              L.msam2_label_clean_workspace_bytes(4) - 1, 2, 4, 4, None),
        "label_clean: null out": lambda: L.msam2_label_clean(ptr, ptr, ptr, ptr, 4, None, 0, None, ptr, ptr, big, 2, 4, 4, None),
        "label_clean: null info": lambda: L.msam2_label_clean(ptr, ptr, ptr, ptr, 4, None, 0, ptr, None, ptr, big, 2, 4, 4, None),
        "label_clean: W": lambda: L.msam2_label_clean(ptr, ptr, ptr, ptr, 4, None, 0, ptr, ptr, ptr, big, 2, 4, 8193, None),
        "label_overlap: n = 0": lambda: L.msam2_label_overlap(ptr, ptr, ptr, 2, 4, 4, 0, ptr, None),
        "label_overlap: n = 33": lambda: L.msam2_label_overlap(ptr, ptr, ptr, 2, 4, 4, 33, ptr, None),
        "label_overlap: null counts": lambda: L.msam2_label_overlap(ptr, ptr, ptr, 2, 4, 4, 4, None, None),
        "label_overlap: voxels": lambda: L.msam2_label_overlap(ptr, ptr, ptr, 33, 8192, 8192, 4, ptr, None),
    }
    for what, call in cases.items():
        rc = call()
        msg = L.msam2_last_error().decode()
        assert rc < 0, (what, rc)
        assert msg.startswith(what.split(":")[0] + ":"), (what, msg)


def test_workspace_sizes_are_zero_exactly_beyond_the_limits():
    """msam2_label_components_workspace_bytes returns 0 for the sizes the entry refuses and only for them: every dimension at its limit and
    one beyond, and the voxel cap (2^31 - 2 = 49981 x 2387 x 18; 2^31 - 1 is prime, so the next volume that exists is 2^31)"""
    from medical_sam2_amd import _lib
    L = _lib.lib()
    ws = L.msam2_label_components_workspace_bytes
    assert ws(1, 1, 1) == 4 and ws(0, 1, 1) == 0 and ws(1, 0, 1) == 0 and ws(1, 1, 0) == 0
    assert ws(65535, 1, 1) == 65535 * 4 and ws(65536, 1, 1) == 0
    assert ws(1, 8192, 1) == 8192 * 4 and ws(1, 8193, 1) == 0
    assert ws(1, 1, 8192) == 8192 * 4 and ws(1, 1, 8193) == 0
    assert ws(49981, 2387, 18) == (2 ** 31 - 2) * 4 and ws(32768, 8192, 8) == 0
    clean = L.msam2_label_clean_workspace_bytes
    assert clean(1) == clean(32) > 0 and clean(0) == 0 and clean(33) == 0


def test_wrappers_check_their_arguments_without_a_device():
    import medical_sam2_amd.ops as ops
    from medical_sam2_amd.volume_labels import clean_labels, label_scores
    vol = torch.zeros(2, 4, 6, dtype=torch.uint8)
    tab = torch.zeros(2, 4, 6, dtype=torch.int32)
    with pytest.raises(ValueError, match="connectivity 5"):
        ops.label_components(vol, 5)
    with pytest.raises(ValueError, match="must be on the GPU"):
        ops.label_components(vol, 26)
    with pytest.raises(ValueError, match="uint8 contiguous"):
        ops.label_components(vol.to(torch.int32))
    with pytest.raises(ValueError, match="uint8 contiguous"):
        ops.label_components(vol[:, :, ::2])
    with pytest.raises(ValueError, match="distinct"):
        ops.label_clean(vol, tab, tab, [3, 3])
    with pytest.raises(ValueError, match="1 .. 255"):
        ops.label_clean(vol, tab, tab, [0, 3])
    with pytest.raises(ValueError, match="got 33"):
        ops.label_clean(vol, tab, tab, list(range(1, 34)))
    with pytest.raises(ValueError, match="must be on the GPU"):
        ops.label_clean(vol, tab, tab, [1, 2])
    with pytest.raises(ValueError, match="must be on the GPU"):
        ops.label_overlap(vol, vol, [1, 2])
    assert ops.label_largest_mask(True, 3) == 0b111 and ops.label_largest_mask(False, 3) == 0 and ops.label_largest_mask(True, 32) == 2 ** 32 - 1
    assert ops.label_largest_mask([True, False, True], 3) == 0b101
    with pytest.raises(ValueError, match="keep_largest names 2"):
        ops.label_largest_mask([True, False], 3)
    with pytest.raises(AssertionError, match="number of objects n"):
        clean_labels(vol)
    with pytest.raises(AssertionError, match="3 ids for n = 2"):
        clean_labels(vol, [1, 2, 3], n=2)
    with pytest.raises(ValueError, match="must be on the GPU"):
        clean_labels(vol, n=2)
    with pytest.raises(ValueError, match="must be on the GPU"):
        label_scores(vol, vol, [1, 2])
