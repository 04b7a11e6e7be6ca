"""Host side of the bodies query (implisolid_layer_bodies' argument checks, implisolid_layer_bodies_copy,
bodies_decode, enclosed_voids, floating_bodies), the restatement tests/np_bodies.py against np_islands on single
layers, and the preconditions of the cases of test_gpu_bodies.py, among them a restatement of the sizing rule of the
stack-wide arrays (body_layers' grow_keeping over engine.hip's block classes) on the run counts of `growing`.  No GPU."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import body_inputs as bi   # noqa: E402
import island_inputs as ii   # noqa: E402
import np_bodies   # noqa: E402
import np_islands   # noqa: E402
import run_inputs as ri   # noqa: E402
import test_cpu_runs as cr   # noqa: E402  (the comb's reference image; its tests are not collected from here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = ii.EYE
UNIT = [-1, 1, -1, 1]

_REST = {}


def restated(name, target, connectivity):
    """(bits, run_offsets, records, runs, decode) of a painted stack, computed once"""
    key = (name, target, connectivity)
    if key not in _REST:
        bits = bi.PAINTED[name]()
        _REST[key] = (bits,) + np_bodies.bodies(bits.astype(np.uint8), 1, target, connectivity)
    return _REST[key]


comb_image = cr.comb_image


def comb_bodies(oracle, s, threshold, target, connectivity):
    """np_bodies.bodies of the comb's reference image, computed once"""
    key = ("comb", s, threshold, target, connectivity)
    if key not in _REST:
        _REST[key] = np_bodies.bodies(comb_image(oracle, s), threshold, target, connectivity)
    return _REST[key]


def voids(name, connectivity):
    bits, offs, rec, runs, dec = restated(name, 0, connectivity)
    L, H, W = bits.shape
    r = rec
    return r[(r[:, 2] > 0) & (r[:, 3] > 0) & (r[:, 4] > 0) & (r[:, 5] < W - 1) & (r[:, 6] < H - 1) & (r[:, 7] < L - 1)]


# ---- the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", sorted(ii.PAINTED))
def test_one_layer_of_the_restatement_is_np_islands(name, connectivity):
    stack = ii.PAINTED[name]()
    for bits in stack[:2]:
        offs, rec, runs, dec = np_bodies.bodies(bits[None].astype(np.uint8), 1, 1, connectivity)
        io, ic, il = np_islands.islands(bits[None].astype(np.uint8), 1, 4 if connectivity == 6 else 8)
        assert np.array_equal(rec[:, 0], ic[:, 0]) and np.array_equal(rec[:, 1], ic[:, 1]), "seeds and areas"
        assert np.array_equal(rec[:, [2, 3, 5, 6]], ic[:, 3:7]) and (rec[:, [4, 7]] == 0).all()
        assert np.array_equal(np.where(dec >= 0, rec[:, 0][dec], -1), il), "the decoded bodies are the island labels"
        assert offs.tolist() == [0, len(runs)] and runs[:, 1].sum() == bits.sum()


def test_the_restatement_s_records_and_runs_on_a_hand_made_stack():
    bits = np.array([[[1, 1, 0, 1], [0, 0, 0, 1]], [[0, 0, 0, 0], [0, 1, 0, 0]]], bool)   # (2, 2, 4)
    offs, rec, runs, dec = np_bodies.bodies(bits.astype(np.uint8), 1, 1, 6)
    assert rec.tolist() == [[0, 2, 0, 0, 0, 1, 0, 0], [3, 2, 3, 0, 0, 3, 1, 0], [13, 1, 1, 1, 1, 1, 1, 1]]
    assert offs.tolist() == [0, 3, 4] and runs.tolist() == [[0, 2, 0], [3, 1, 1], [7, 1, 1], [5, 1, 2]]
    offs, rec, runs, dec = np_bodies.bodies(bits.astype(np.uint8), 1, 1, 26)
    assert rec.tolist() == [[0, 3, 0, 0, 0, 1, 1, 1], [3, 2, 3, 0, 0, 3, 1, 0]], "(1, 1, 1) touches (0, 0, 0) and (0, 0, 1) by a corner and an edge"
    assert runs[:, 2].tolist() == [0, 1, 1, 0] and dec[1, 1].tolist() == [-1, 0, -1, -1]
    offs, rec, runs, dec = np_bodies.bodies(bits.astype(np.uint8), 1, 0, 6)
    assert len(rec) == 1 and rec[0].tolist() == [2, 11, 0, 0, 0, 3, 1, 1] and offs.tolist() == [0, 2, 5]
    assert runs.tolist() == [[2, 1, 0], [4, 3, 0], [0, 4, 0], [4, 1, 0], [6, 2, 0]]


# ---- the painted stacks are what they say --------------------------------------------------------------------------
def test_every_painted_stack_fits_the_table_limits():
    for name, make in bi.PAINTED.items():
        node, rect, z = ii.painted(make())
        assert len(z) == make().shape[0], name
    for W in bi.SIZES:
        for H in bi.SIZES:
            for L in bi.LAYERS:
                assert bi.sized(W, H, L).shape == (L, H, W)
    assert bi.sized(17, 15, 3).any() and not bi.sized(17, 15, 3).all()


def test_the_arch_is_one_body_only_through_its_bridge():
    for conn in (6, 26):
        assert len(restated("arch", 1, conn)[2]) == 1
        assert len(restated("arch_open", 1, conn)[2]) == 2
        assert len(restated("arch_bottom", 1, conn)[2]) == 1
        top = restated("arch", 1, conn)[2][0]
        assert top.tolist() == [20 * 70 + 2, 10 + 64, 2, 20, 0, 67, 20, 4]
        # the pillars meet only in the last layer: every layer below holds two row runs that belong to one body
        offs, runs = restated("arch", 1, conn)[1], restated("arch", 1, conn)[3]
        assert np.diff(offs).tolist() == [2, 2, 2, 2, 1] and (runs[:, 2] == 0).all()
    assert not bi.arch()[:4, :, 3:67].any() and 67 // 64 != 2 // 64, "the pillars stand in different 64-pixel column blocks"


def test_the_contacts_split_by_kind():
    bits = bi.contacts()
    pairs = bi.contact_pairs()
    assert len(pairs) == 26 and bits.sum() == 52
    kinds = {1: 0, 2: 0, 3: 0}
    for d, a, b in pairs:
        kinds[sum(abs(v) for v in d)] += 1
        assert {a[2], b[2]} <= {63, 64} and (a[1] in (0, bits.shape[1] - 1) or b[1] in (0, bits.shape[1] - 1))
    assert kinds == {1: 6, 2: 12, 3: 8}, "faces, edges and corners, each in row 0 and in the last row"
    dec6, dec26 = restated("contacts", 1, 6)[4], restated("contacts", 1, 26)[4]
    for d, a, b in pairs:
        assert (dec6[a] == dec6[b]) == (sum(abs(v) for v in d) == 1), d
        assert dec26[a] == dec26[b], d
    assert len(restated("contacts", 1, 6)[2]) == 2 * (3 + 2 * 10) and len(restated("contacts", 1, 26)[2]) == 26
    across = {tuple(int(v != 0) for v in d) for d, _, _ in pairs}
    assert across == {(0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)}, "layers, rows, columns and all their combinations"
    assert ((1, 1, -1) in bi.HALF) and ((1, -1, 0) in bi.HALF) and ((1, -1, 1) in bi.HALF), "the rows py - 1 and py + 1 of the layer below"


def test_the_helix_is_one_long_path():
    bits = bi.helix()
    assert bits.shape == (4, 33, 65)
    for conn in (6, 26):
        _, offs, rec, runs, dec = restated("helix", 1, conn)
        assert len(rec) == 1 and rec[0].tolist() == [0, int(bits.sum()), 0, 0, 0, 64, 32, 3]
    # a path: under 6 every voxel has two neighbours but the two ends
    p = np.pad(bits, 1)
    n = sum(p[1 + dl:5 + dl, 1 + dy:34 + dy, 1 + dx:66 + dx] for dl, dy, dx in np_bodies.STEPS6)
    assert sorted(np.unique(n[bits]).tolist()) == [1, 2] and int((n[bits] == 1).sum()) == 2
    assert bits.sum() == 17 * 65 + 16 * 2 and len(runs) == 17 + 32


def test_the_cavities_hold_the_stated_voids():
    bits = bi.cavities()
    assert bits.shape == (7, 24, 24)
    _, offs, rec6, runs, dec = restated("cavities", 0, 6)
    assert len(rec6) == 5
    by_seed = {int(r[0]): r for r in rec6}
    key = lambda l, y, x: (l * 24 + y) * 24 + x   # noqa: E731
    A, B, C, D, E = key(2, 3, 3), key(4, 3, 10), key(3, 12, 0), key(2, 16, 16), key(4, 19, 19)
    assert sorted(by_seed) == sorted([A, B, C, D, E])
    assert [int(by_seed[k][1]) for k in (A, B, C, D, E)] == [18, 27, 10, 18, 12]
    v6 = voids("cavities", 6)
    assert sorted(v6[:, 0].tolist()) == sorted([A, D]), "under 6 the corner contact seals D"
    rec26 = restated("cavities", 0, 26)[2]
    assert len(rec26) == 4 and sorted(rec26[:, 0].tolist()) == sorted([A, B, C, D])
    assert [r for r in rec26 if r[0] == D][0].tolist() == [D, 30, 16, 16, 2, 20, 20, 6], "under 26 D drains through the shaft"
    assert voids("cavities", 26)[:, 0].tolist() == [A]
    assert not bits[3, 18, 18] and not bits[4, 19, 19] and bits[3, 19, 19] and bits[4, 18, 18] and bits[3, 18, 19] and bits[3, 19, 18]
    for conn in (6, 26):
        assert len(restated("cavities", 1, conn)[2]) == 1, "the block stays one solid body"


def test_the_floating_stack_holds_a_loose_part_and_a_part_that_joins():
    bits = bi.floating()
    for conn in (6, 26):
        _, offs, rec, runs, dec = restated("floating", 1, conn)
        assert len(rec) == 2
        assert rec[0].tolist() == [2 * 20 + 2, 80 + 36 + 3, 2, 2, 0, 11, 5, 4]
        assert rec[1].tolist() == [(2 * 20 + 12) * 20 + 12, 18, 12, 12, 2, 14, 14, 3]
        assert [r[4] for r in rec if r[4] > 0] == [2], "only the loose block floats"
    # the part is an island of layer 1: nothing of layer 0 under it, and its own component in that layer
    io, ic, il = np_islands.islands(bits.astype(np.uint8), 1, 8)
    l1 = ic[io[1]:io[2]]
    assert len(l1) == 2 and sorted(l1[:, 2].tolist()) == [0, 16]
    assert not bits[:3, :, 6:9].any() and bits[3, 3, 6:9].all(), "it joins in layer 3 only"


def test_the_dense_rows_hold_more_runs_than_a_wave():
    bits = bi.dense_rows()
    assert bits.shape == (3, 3, 130)
    _, offs, rec, runs, dec = restated("dense_rows", 1, 6)
    assert len(runs) == 9 * 65 and np.diff(offs).tolist() == [195, 195, 195] and 65 > 64
    assert len(rec) == bits.sum() == 585 and (rec[:, 1] == 1).all(), "under 6 every voxel is its own body"
    assert len(restated("dense_rows", 1, 26)[2]) == 1
    e = restated("dense_rows", 0, 6)
    assert len(e[3]) == 9 * 65 and len(e[2]) == 585, "and so is every empty voxel"


def test_the_random_stacks_have_many_bodies_of_both_classes():
    for name in ("random_50", "random_60"):
        for target in (0, 1):
            n6, n26 = len(restated(name, target, 6)[2]), len(restated(name, target, 26)[2])
            assert n6 > n26 >= 1 and n6 > 20, (name, target, n6, n26)
            _, offs, rec, runs, dec = restated(name, target, 26)
            assert (rec[:, 7] > rec[:, 4]).any() and rec[:, 1].sum() == (dec >= 0).sum()


def test_the_empty_and_full_stacks():
    for conn in (6, 26):
        assert len(restated("empty", 1, conn)[2]) == 0 and len(restated("full", 0, conn)[2]) == 0
        assert restated("empty", 1, conn)[1].tolist() == [0, 0, 0, 0]
        for name, target in (("empty", 0), ("full", 1)):
            _, offs, rec, runs, dec = restated(name, target, conn)
            assert rec.tolist() == [[0, 3 * 17 * 65, 0, 0, 0, 64, 16, 2]] and len(runs) == 3 * 17 and (runs[:, 1] == 65).all()


def test_the_chunked_stack_joins_bodies_across_the_chunk_borders():
    bits, offs, rec, runs, dec = restated("chunked", 1, 26)
    assert bits.shape == (12, 40, 40)
    for first in (4, 8):   # the first layers of the chunks of four
        below, above = dec[first - 1], dec[first]
        both = (below >= 0) & (above >= 0)
        assert both.any() and np.array_equal(below[both], above[both]), "bodies run through the border"
    assert (rec[:, 4] < 4).any() and (rec[:, 7] >= 8).any() and len(rec) > 3
    assert any(r[4] == 4 for r in rec) or any(r[4] == 8 for r in rec), "a body that starts on a chunk's first layer"


# ---- a stack that outgrows its arrays ----------------------------------------------------------------------------
def pool_class(n):
    """engine.hip's block sizes: at least 256 bytes, then eighths of an octave (5, 6, 7, 8 eighths of a power of two)"""
    c = 256
    while c < n:
        c <<= 1
    q = c >> 3
    for k in (5, 6, 7, 8):
        if n <= q * k and q * k >= 256:
            return q * k
    return c


def regrowths(counts, item):
    """body_layers' sizing of one stack-wide array of `item` bytes a run over chunks of counts[k] runs, from an empty
    buffer: [(bytes kept, new block's bytes)] of every chunk that takes another block.  grow_keeping leaves a block
    that holds total + cc + 1 entries; otherwise the new one is the class of max(want, 1.5 x bytes) and the first
    `total` entries are copied over"""
    out, size, total = [], 0, 0
    for cc in counts:
        want = (total + cc + 1) * item
        if not (size and want <= size):
            size = pool_class(max(want, size + size // 2, 256))
            out.append((total * item, size))
        total += cc
    return out


GROWING_CASES = [(1, 26), (0, 6)]   # what test_gpu_bodies.py runs in a process of its own
GROWING_REGROWTHS = {}              # (target, connectivity) -> (of the runs, of the union-find), with bytes kept


def test_the_sizing_rule_s_restatement():
    assert [pool_class(n) for n in (1, 256, 257, 320, 321, 384, 449, 512, 513, 641, 1025)] == [256, 256, 320, 320, 384, 384, 512, 512, 640, 768, 1280]
    assert regrowths([10], 8) == [(0, 256)] and regrowths([31, 1], 8) == [(0, 256), (248, 384)]
    assert regrowths([31, 0, 16, 1], 8) == [(0, 256), (248, 384), (376, 640)], "a block that still fits is left; 1.5 x 384 = 576 is of the class 640"
    assert regrowths([10, 200], 4) == [(0, 256), (40, 896)], "a chunk beyond 1.5 x: the class of what it needs"


@pytest.mark.parametrize("target, connectivity", GROWING_CASES)
def test_the_growing_stack_outgrows_its_arrays_chunk_by_chunk(target, connectivity):
    bits, offs, rec, runs, dec = restated("growing", target, connectivity)
    L, H, W = bits.shape
    assert L == 10 and H <= 24 and W <= 64
    counts = np.diff(offs).tolist()
    assert all(b > a for a, b in zip(counts, counts[1:])), "the run count rises from layer to layer"
    grown = [regrowths(counts, item) for item in (8, 4)]   # int32 {x0, x1} and the int32 parent, a layer per chunk
    kept = [sum(1 for keep, size in g if keep > 0) for g in grown]
    GROWING_REGROWTHS[(target, connectivity)] = kept
    print("growing", target, connectivity, "runs per layer", counts, "blocks taken with bytes kept: runs", kept[0], grown[0], "parent", kept[1], grown[1])
    assert min(kept) >= 3 and all(g[0][0] == 0 for g in grown), "both arrays move at least three times with earlier chunks' entries in them"
    assert grown[0][-1][0] > 0 and len(grown[0]) > L // 2, "and still in the second half of the stack"


@pytest.mark.parametrize("connectivity", [6, 26])
def test_the_growing_stack_holds_the_stated_bodies(connectivity):
    bits, offs, rec, runs, dec = restated("growing", 1, connectivity)
    L, H, W = bits.shape
    by_seed = {int(r[0]): r.tolist() for r in rec}
    key = lambda l, y, x: (l * H + y) * W + x   # noqa: E731
    # the pillar: the stack's first run is its root, and the last layer still adds runs to it
    assert by_seed[0] == [0, 4 * L, 0, 0, 0, 1, 1, L - 1] and runs[0].tolist() == [0, 2, 0]
    assert runs[offs[L - 1]].tolist() == [0, 2, 0] and runs[offs[L - 1] + 1].tolist() == [W, 2, 0]
    assert by_seed[key(0, 3, 10)] == [key(0, 3, 10), 2 * 15, 10, 3, 0, 14, 5, 1], "a body that ends in layer 1"
    assert by_seed[key(7, 3, 30)] == [key(7, 3, 30), 3 * 15, 30, 3, 7, 34, 5, 9], "a body that starts in layer 7"
    # the pair: its second pillar's runs of the first layers are written by the first chunk and hang on x = 40's only
    # through the bar of the last layer
    assert by_seed[key(0, 22, 40)] == [key(0, 22, 40), 2 * (L - 1) + 21, 40, 22, 0, 60, 22, L - 1] and key(0, 22, 60) not in by_seed
    assert not bits[:L - 1, 21:24, 41:60].any() and bits[L - 1, 22, 40:61].all()
    assert dec[0, 22, 60] == dec[0, 22, 40] == dec[L - 1, 22, 50]
    open_ = np_bodies.bodies(np.where(np.arange(L)[:, None, None] < L - 1, bits, False).astype(np.uint8), 1, 1, connectivity)
    assert open_[3][0, 22, 60] != open_[3][0, 22, 40], "without the last layer they are two bodies"
    assert len(rec) > 30 and (rec[:, 4] > 0).sum() > 20, "and the single pixels start bodies in every layer"


# ---- rows of two full steps and more ---------------------------------------------------------------------------------
DENSE = ["dense_511", "dense_512", "dense_512_ends"]


def _row_runs(offs, runs, H, W):
    """the run records of every row of the stack: {(l, py): int32 (n, 3)}"""
    out = {}
    for l in range(len(offs) - 1):
        r = runs[offs[l]:offs[l + 1]]
        for py in range(H):
            out[(l, py)] = r[r[:, 0] // W == py]
    return out


@pytest.mark.parametrize("name", DENSE)
def test_the_dense_rows_fill_both_steps_and_more_than_a_round(name):
    bits = bi.PAINTED[name]()
    L, H, W = bits.shape
    assert (L, H) == (2, 3) and W in (511, 512) and 256 < W <= 512, "two steps of the walk; 512 is the table's limit"
    for target in (0, 1):
        on = bits == (target == 1)
        for l in range(L):
            for py in range(H):
                starts = ri.step_starts(on[l, py])
                assert len(starts) == 2 and min(starts) >= 40, (name, target, l, py, starts)
                assert sum(starts) > 64, "more than one round of 64 runs in every row, of each class"
                first = on[l, py] & ~np.concatenate(([False], on[l, py, :-1]))
                assert len(set((np.flatnonzero(first[256:]) // 4).tolist())) >= 16, "starts in many lanes of the second step"
    if name == "dense_512_ends":
        assert bits[0, :, 511].all() and not bits[1, :, 511].any(), "a last pixel of each class in every row, behind a full step of ends"
        assert ri.step_starts(bits[0, 1])[0] > 64 and sum(ri.step_starts(bits[0, 1])) > 128, "three rounds of 64 runs in a row"
        assert sum(ri.step_starts(~bits[0, 1])) > 128
    if W == 512:
        assert any(bits[l, py, 511] for l in range(L) for py in range(H)) and not all(bits[l, py, 511] for l in range(L) for py in range(H))


def test_some_dense_row_holds_more_than_128_solid_runs():
    assert max(sum(ri.step_starts(row)) for name in DENSE for layer in bi.PAINTED[name]() for row in layer) > 128


@pytest.mark.parametrize("name", DENSE)
def test_long_dense_rows_hold_runs_of_many_bodies(name):
    # under 6 a row of more than 64 runs holds runs of three and more bodies: the tally's step of mixed bodies
    bits, offs, rec, runs, dec = restated(name, 1, 6)
    rows = _row_runs(offs, runs, 3, bits.shape[2])
    assert all(len(r) > 64 and len(set(r[:, 2].tolist())) >= 3 for r in rows.values())


def test_the_rounds_stack_gathers_a_body_over_rounds_and_rows_and_then_mixes():
    bits, offs, rec, runs, dec = restated("rounds", 1, 6)
    rows = _row_runs(offs, runs, 2, 512)
    kinds = {k: [sorted(set(r[i:i + 64, 2].tolist())) for i in range(0, len(r), 64)] for k, r in rows.items()}
    assert [len(rows[k]) for k in sorted(rows)] == [1, 256, 1, 1 + 55]
    # the tally's wave takes the four rows in turn: row 0's run and two whole rounds of row 1 are of body 0 ...
    assert kinds[(0, 0)] == [[0]] and kinds[(0, 1)][:2] == [[0], [0]]
    # ... the third round holds it beside bodies of its own, the fourth only such bodies ...
    assert len(kinds[(0, 1)]) == 4 and kinds[(0, 1)][2][0] == 0 and len(kinds[(0, 1)][2]) == 1 + 42 and len(kinds[(0, 1)][3]) == 64
    assert (rows[(0, 1)][:150, 2] == 0).all() and (rows[(0, 1)][150:, 2] > 0).all()
    # ... the bar is another body in a step of its own, and the last row comes back to body 0 with others behind it
    assert kinds[(1, 0)] != [[0]] and len(kinds[(1, 0)][0]) == 1 and rec[kinds[(1, 0)][0][0]].tolist() == [1024 + 401, 3, 401, 0, 1, 403, 0, 1]
    assert rows[(1, 1)][:3, 2].tolist() == [0, 0, 0] and len(kinds[(1, 1)][0]) == 1 + 53
    # the neighbour row of more than 64 runs: the runs of layer 1 bisect row (0, 1)'s 256
    assert rows[(1, 1)][0].tolist() == [512, 290, 0] and len(rec) == 1 + 106 + 1
    assert 1 < len(restated("rounds", 1, 26)[2]) < len(rec), "under 26 the bar and the pixel at x = 300 touch body 0 by a corner"


def test_the_comb_fills_every_step_and_straddles_every_seam(oracle):
    cov = comb_image(oracle, 1)
    W, H = ri.COMB_W, ri.COMB_H
    assert cov.shape == (2, H, W) and W == 4 * 256 + 6 and len(ri.COMB_TEETH) == 34
    on = cov[0, 1] >= 1
    solid, empty = ri.step_starts(on), ri.step_starts(~on)
    print("comb, the middle row of plane 0: solid and empty starts per step", solid, empty)
    # the last step holds six pixels: at most three starts of one class, so its count is of both classes
    assert len(solid) == 5 and min(solid[:4]) >= 4 and min(empty[:4]) >= 4 and solid[4] >= 2 and empty[4] >= 2 and solid[4] + empty[4] >= 4
    for x in ri.COMB_SEAMS:
        assert on[x - 1] and on[x] and not on[x - 2] and not on[x + 1], "a tooth of two pixels on the seam"
        assert not (cov[0, 0, x - 8:x + 8] >= 1).any() and not (cov[0, 2, x - 8:x + 8] >= 1).any(), "and an empty run across it above and below"
    for conn in (6, 26):
        offs, rec, runs, dec = comb_bodies(oracle, 1, 1, 0, conn)
        assert len(rec) == 1 and rec[0].tolist() == [0, int((cov < 1).sum()), 0, 0, 0, W - 1, H - 1, 1], "the empty class is one body"
        offs, rec, runs, dec = comb_bodies(oracle, 1, 1, 1, conn)
        assert len(rec) == len(ri.COMB_TEETH), "and every tooth a solid body"
    grey = comb_image(oracle, 2)
    assert 1 < int(grey[grey < 4].max()) and int(grey.max()) == 4, "grey values beyond 0 / 1"


# ---- the ABI ---------------------------------------------------------------------------------------------------
def test_abi_declares_the_body_entries(impli):
    L = impli.lib()
    header = open(os.path.join(ROOT, "include", "implisolid.h")).read()
    for name, decl in (("implisolid_layer_bodies", "int64_t implisolid_layer_bodies("),
                       ("implisolid_layer_bodies_copy", "int implisolid_layer_bodies_copy(int64_t* bodies, int32_t* runs)"),
                       ("implisolid_debug_layer_bodies_ms", "int implisolid_debug_layer_bodies_ms(int enable, double ms[4])")):
        assert hasattr(L, name) and name in impli.ABI_SYMBOLS and decl in header, name
    for word in ("target", "connectivity", "want_runs", "run_offsets", "seed", "volume", "IMPLISOLID_BODIES_CHUNK", "2^31 row runs"):
        assert word in header, word
    assert impli.BODY_DTYPE.names == np_bodies.FIELDS and impli.BODY_DTYPE.itemsize == 64
    assert impli.BODY_RUN_DTYPE.names == np_bodies.RUN_FIELDS and impli.BODY_RUN_DTYPE.itemsize == 12


fp = ctypes.POINTER(ctypes.c_float)
lp = ctypes.POINTER(ctypes.c_int64)
ip = ctypes.POINTER(ctypes.c_int32)
SPHERE = json.dumps({"type": "iellipsoid", "matrix": EYE}).encode()
NO_COPY = "implisolid_layer_bodies_copy: no bodies to copy (the last implisolid_layer_bodies failed, or none ran)"
WHO = "implisolid_layer_bodies: "
REFUSALS = [
    (dict(n=0), WHO + "n_layers must be in [1, 65536]"),
    (dict(n=65537), WHO + "n_layers must be in [1, 65536]"),
    (dict(z=[0.0, np.nan]), WHO + "every z must be finite"),
    (dict(W=0), WHO + "width and height must be in [1, 16384]"),
    (dict(H=16385), WHO + "width and height must be in [1, 16384]"),
    (dict(s=3), WHO + "supersample must be 1, 2 or 4"),
    (dict(threshold=0), WHO + "threshold must be in [1, supersample^2]"),
    (dict(threshold=5), WHO + "threshold must be in [1, supersample^2]"),
    (dict(s=1, threshold=2), WHO + "threshold must be in [1, supersample^2]"),
    (dict(target=2), WHO + "target must be 0 (empty) or 1 (solid)"),
    (dict(target=-1), WHO + "target must be 0 (empty) or 1 (solid)"),
    (dict(connectivity=8), WHO + "connectivity must be 6 or 26"),
    (dict(connectivity=18), WHO + "connectivity must be 6 or 26"),
    (dict(want_runs=2), WHO + "want_runs must be 0 or 1"),
    (dict(want_runs=-1), WHO + "want_runs must be 0 or 1"),
    (dict(rect=[1, -1, -1, 1]), "raster: the rect must be finite with min < max on both axes"),
    (dict(rect=[-1, 1, -np.inf, 1]), "raster: the rect must be finite with min < max on both axes"),
    (dict(shape=b'{"type": "iellipsoid", "matrix": [1, 0'), "JSON parse error: expected , or ]"),
    (dict(shape=json.dumps({"type": "no_such_solid", "matrix": EYE}).encode()), 'Invalid object you asked for: "no_such_solid"'),
    (dict(shape=None), WHO + "bad arguments"),
    (dict(offsets=None), WHO + "bad arguments"),
    # the documented order: implisolid_islands' (n_layers, z, width / height, supersample, threshold), then target,
    # connectivity, want_runs, the rect, and the shape last -- nothing is compiled for a bad request
    (dict(n=0, z=[np.nan, 0.0], W=0), WHO + "n_layers must be in [1, 65536]"),
    (dict(z=[np.nan, 0.0], W=0, s=3), WHO + "every z must be finite"),
    (dict(W=0, s=3, threshold=0), WHO + "width and height must be in [1, 16384]"),
    (dict(s=3, threshold=0, target=2), WHO + "supersample must be 1, 2 or 4"),
    (dict(threshold=0, target=2, connectivity=4), WHO + "threshold must be in [1, supersample^2]"),
    (dict(target=2, connectivity=4, want_runs=2), WHO + "target must be 0 (empty) or 1 (solid)"),
    (dict(connectivity=4, want_runs=2, rect=[1, -1, -1, 1]), WHO + "connectivity must be 6 or 26"),
    (dict(want_runs=2, rect=[1, -1, -1, 1], shape=b"{"), WHO + "want_runs must be 0 or 1"),
    (dict(rect=[1, -1, -1, 1], shape=b"{"), "raster: the rect must be finite with min < max on both axes"),
    (dict(shape=b"{", offsets=None), WHO + "bad arguments"),
]


def _call(L, kw):
    n = kw.get("n", 2)
    z = np.zeros(max(n, 2), np.float32) if "z" not in kw else np.array(kw["z"], np.float32)
    rect = np.array(kw.get("rect", UNIT), np.float32)
    offs = np.zeros(max(n, 2) + 1, np.int64)
    return L.implisolid_layer_bodies(kw.get("shape", SPHERE), 0, rect.ctypes.data_as(fp), kw.get("W", 8), kw.get("H", 8), kw.get("s", 2),
                                     z.ctypes.data_as(fp), n, kw.get("threshold", 1), kw.get("target", 1), kw.get("connectivity", 26),
                                     kw.get("want_runs", 0), None if "offsets" in kw else offs.ctypes.data_as(lp), None)


def _copy_refuses(impli):
    L = impli.lib()
    bodies, runs = np.zeros(8, np.int64), np.zeros(3, np.int32)
    assert L.implisolid_layer_bodies_copy(bodies.ctypes.data_as(lp), runs.ctypes.data_as(ip)) == -1 and impli.last_error() == NO_COPY
    assert L.implisolid_layer_bodies_copy(bodies.ctypes.data_as(lp), None) == -1 and impli.last_error() == NO_COPY
    assert L.implisolid_layer_bodies_copy(None, None) == -1 and impli.last_error() == NO_COPY


def test_copy_refuses_with_an_empty_slot(impli):
    # whatever ran before in this process, a refused call leaves the slot empty
    assert _call(impli.lib(), dict(n=0)) == -1
    _copy_refuses(impli)


@pytest.mark.parametrize("kw, message", REFUSALS)
def test_bad_input_is_refused_before_a_device_and_empties_the_slot(impli, kw, message):
    L = impli.lib()
    assert _call(L, kw) == -1
    assert impli.last_error() == message
    _copy_refuses(impli)
    # the same refusal straight after a refused call
    assert _call(L, kw) == -1 and impli.last_error() == message
    assert impli.raster_coords(UNIT, 8, 8, 2)[0].shape == (16,) and impli.last_error() == "", "and the next call works"


@pytest.mark.parametrize("kw", [dict(width=0), dict(height=16385), dict(z=[]), dict(z=[np.inf]), dict(supersample=3), dict(threshold=0),
                                dict(supersample=2, threshold=5), dict(target=2), dict(connectivity=8), dict(rect=[1, -1, -1, 1])])
def test_the_python_entry_refuses_them_too(impli, kw):
    a = dict(shape=json.loads(SPHERE), rect=UNIT, width=8, height=8, z=[0.0, 0.1])
    a.update(kw)
    with pytest.raises(impli.ImplisolidError) as e:
        impli.layer_bodies(**a)
    assert str(e.value)
    with pytest.raises(ValueError):
        impli.layer_bodies(json.loads(SPHERE), [0, 1, 2], 8, 8, [0.0])


def test_the_timer_answers_without_a_call(impli):
    ms = impli.layer_bodies_kernel_ms(False)
    assert len(ms) == 4


# ---- the host helpers ------------------------------------------------------------------------------------------------
def test_bodies_decode_on_hand_made_runs(impli):
    # two layers of 3 rows x 5 columns
    offs = np.array([0, 3, 4], np.int64)
    rows = np.array([[0, 2, 0], [3, 2, 1], [12, 3, 1], [5, 5, 0]], np.int32)
    runs = np.ascontiguousarray(rows).view(impli.BODY_RUN_DTYPE).reshape(-1)
    want = np.full((2, 3, 5), -1, np.int32)
    want[0, 0, 0:2] = 0
    want[0, 0, 3:5] = 1
    want[0, 2, 2:5] = 1
    want[1, 1, :] = 0
    for given in (runs, rows):
        got = impli.bodies_decode(offs, given, 5, 3)
        assert got.dtype == np.int32 and np.array_equal(got, want)
    assert (impli.bodies_decode([0, 0, 0], np.zeros((0, 3), np.int32), 5, 3) == -1).all()
    for bad_offs, bad_rows in (([0, 3], rows), ([0, 5, 4], rows), ([0, 3, 4], [[0, 2, 0], [3, 3, 1], [12, 3, 1], [5, 5, 0]]),
                               ([0, 3, 4], [[0, 0, 0], [3, 2, 1], [12, 3, 1], [5, 5, 0]]), ([0, 3, 4], [[0, 2, 0], [3, 2, 1], [15, 3, 1], [5, 5, 0]])):
        with pytest.raises(ValueError):
            impli.bodies_decode(bad_offs, np.array(bad_rows, np.int32), 5, 3)


def test_bodies_decode_inverts_the_restatement_s_runs(impli):
    for name, target in (("cavities", 0), ("random_50", 1), ("dense_rows", 1)):
        bits, offs, rec, runs, dec = restated(name, target, 26)
        assert np.array_equal(impli.bodies_decode(offs, runs, bits.shape[2], bits.shape[1]), dec), name


def test_enclosed_voids_and_floating_bodies(impli):
    W, H, L = 10, 8, 5
    rows = np.array([
        [0, 100, 0, 0, 0, 9, 7, 4],        # touches everything
        [111, 8, 1, 1, 1, 8, 6, 3],        # touches nothing: the largest box that is still enclosed
        [120, 8, 0, 1, 1, 8, 6, 3],        # x0 = 0
        [121, 8, 1, 0, 1, 8, 6, 3],        # y0 = 0
        [122, 8, 1, 1, 0, 8, 6, 3],        # l0 = 0
        [123, 8, 1, 1, 1, 9, 6, 3],        # x1 = W - 1
        [124, 8, 1, 1, 1, 8, 7, 3],        # y1 = H - 1
        [125, 8, 1, 1, 1, 8, 6, 4],        # l1 = L - 1
        [200, 1, 4, 4, 2, 4, 4, 2],        # a single voxel inside
    ], np.int64)
    bodies = np.ascontiguousarray(rows).view(impli.BODY_DTYPE).reshape(-1)
    for given in (bodies, rows):
        v = impli.enclosed_voids(given, W, H, L)
        assert v.dtype == impli.BODY_DTYPE and v["seed"].tolist() == [111, 200]
        f = impli.floating_bodies(given)
        assert f.dtype == impli.BODY_DTYPE and f["seed"].tolist() == [111, 120, 121, 123, 124, 125, 200]
    assert len(impli.enclosed_voids(bodies[:1], W, H, L)) == 0 and len(impli.floating_bodies(bodies[:1])) == 0
    assert np.array_equal(np_bodies.as_rows(bodies), rows)
    # on the restatement's records of the cavities
    for conn, n in ((6, 2), (26, 1)):
        rec = restated("cavities", 0, conn)[2]
        assert np.array_equal(np_bodies.as_rows(impli.enclosed_voids(rec, 24, 24, 7)), voids("cavities", conn)) and len(voids("cavities", conn)) == n
    assert impli.floating_bodies(restated("floating", 1, 26)[2])["l0"].tolist() == [2]
