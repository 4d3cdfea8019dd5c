"""k_sort_read's row-bounded rounds and its rank phase at the sizes where the
instruction streams change, by the method of test_filtered_sort_parity:
production mode, sort_small 1, the anchors the DP runs on against the oracle's
sorted anchors minus the singletons.

The block-wide passes run whole rows of NT keys in rounds of 16 / 8 / 4 / 2 / 1
rows and a partly filled last row on its own (NT 1024, or 512 at sort_lds_kb
76), so the reads are built on the CPU to put the anchor count A0 at the round
edges: ceil(A0 / 1024) in {1, 2, 8, 9, 16, 17, 24, 25}, each once with a nearly
empty and once with a nearly full last row, and one read close to the 65,535
limit.  A read is a concatenation of dense-world reads truncated base by base
until A0 (the oracle's anchor count at mid_occ 5000) falls in the class."""
import numpy as np
import pytest

import minimap2_rs_amd as M
from oracle import oracle as O
from tools import simdata
from tests.gpu_common import _singleton_keep, dense_world, knobs, small_world  # noqa: F401

pytestmark = pytest.mark.gpu

MID = 5000
ROWS = (1, 2, 8, 9, 16, 17, 24, 25)
ROWS_REQUIRED = (1, 2, 8, 9, 16, 17)
SEG_LENS = (1, 2, 16, 17, 64, 65)


@pytest.fixture(scope="module")
def dev():
    d = M.Device(0)
    yield d
    d.close()


def _n_anchors(oi, q):
    return len(oi.anchors(q, 10, 15, MID)[0]) if len(q) >= 15 else 0


GRID = 512


def _truncate_to(oi, seq, grid, lo, hi):
    """A prefix of seq with lo <= A0 <= hi, or None.  grid[j] = A0(seq[:j * GRID]);
    A0 rises with the length except where a minimizer window takes an anchor back,
    so the first length reaching lo is bisected inside its grid step."""
    j = next((j for j in range(1, len(grid)) if grid[j] >= lo), None)
    if j is None:
        return None
    a, b = (j - 1) * GRID, min(len(seq), j * GRID)
    while a < b:
        m = (a + b) // 2
        if _n_anchors(oi, seq[:m]) < lo:
            a = m + 1
        else:
            b = m
    for m in range(a, min(len(seq), a + 8) + 1):
        if lo <= _n_anchors(oi, seq[:m]) <= hi:
            return seq[:m]
    return None


def _seg_lengths(a):
    """Sizes of the kept cells (the rank phase's segments) of one read's anchors: the 32 kb cell rule of _singleton_keep."""
    if len(a) < 2:
        return np.zeros(0, np.int64)
    a = a[_singleton_keep(a)]
    x = a[:, 0]
    hi = x >> np.uint64(32)
    gid = np.where(hi == np.uint64(0xffffffff), np.uint64(1 << 33), hi)
    cell = (gid << np.uint64(20)) | ((x & np.uint64(0x7fffffff)) >> np.uint64(15))
    return np.unique(cell, return_counts=True)[1]


@pytest.fixture(scope="module")
def world(small_world, dense_world):
    ref, _, _, rseqs = dense_world
    oi = O.OIndex.build(ref, 10, 15, 14, 0, 4)
    idx = M.Index.build_index_from_fasta(ref, 10, 15, 14, 0, 4)
    contigs = simdata.read_fasta_seqs(ref)[1]
    return oi, idx, list(rseqs), list(small_world[3][:3]), contigs


def _wants(oi, qs):
    """The oracle's sorted anchors minus the singletons, per read (computed once per set of reads)."""
    out = []
    for q in qs:
        want, _ = oi.anchors(q, 10, 15, MID)
        out.append(want[_singleton_keep(want)] if len(want) > 1 else want)
    return out


def _check(dev, idx, qs, wants, what):
    dev.upload_index(idx, MID)
    dev.set_debug(False)
    dev.set_reads(qs)
    dev.map(M.map_opts())
    for r, (q, want) in enumerate(zip(qs, wants)):
        got = dev.debug_anchors(r)
        assert np.array_equal(got, want), (what, r, len(q), len(got), len(want))


@pytest.fixture(scope="module")
def row_reads(world):
    """Prefixes of two concatenations of dense-world reads: a unique-sequence
    read and the reads in the segmental duplication (an anchor, or about twelve,
    per minimizer, so that A0 moves in steps well under the 64 of a class)."""
    oi, _, rseqs, spacers, _ = world
    seqs = [rseqs[16] + rseqs[17], b"".join(rseqs[8:16])]
    grids = [[_n_anchors(oi, s[:j * GRID]) for j in range((len(s) + GRID - 1) // GRID + 1)] for s in seqs]
    classes = []
    for rows in ROWS:
        base = (rows - 1) * 1024
        classes += [(rows, "low", max(2, base + 1), base + 64), (rows, "high", base + 960, base + 1024)]
    classes.append((64, "limit", 60000, 65535))
    reads, reached = [], []
    for rows, name, lo, hi in classes:
        for s, g in zip(seqs, grids):
            q = _truncate_to(oi, s, g, lo, hi)
            if q is not None:
                reads.append(q)
                reached.append((rows, name, _n_anchors(oi, q)))
                break
    reads += spacers                          # small-world reads: next to no anchors here
    return reads, reached, _wants(oi, reads)


@pytest.mark.parametrize("seed_fuse,lds_kb", [(1, 0), (0, 0), (1, 76), (0, 76)])
def test_sort_row_edges(dev, world, row_reads, seed_fuse, lds_kb):
    """Fused (seed_fuse 1) and plain P1, P2 and the window gathers at the round
    edges, with 1024 rows (sort_lds_kb 0) and with 512 rows and several windows
    per read (76)."""
    idx = world[1]
    reads, reached, wants = row_reads
    print("classes reached (rows of 1024, last row, A0):", reached)
    missing = [(r, n) for r in ROWS_REQUIRED for n in ("low", "high") if (r, n) not in {(a, b) for a, b, _ in reached}]
    assert not missing, f"anchor-count classes not reached: {missing}; reached {reached}"
    assert any(n == "limit" for _, n, _ in reached), f"no read with 60,000-65,535 anchors; reached {reached}"
    with knobs(dev, sort_small=1, seed_fuse=seed_fuse, sort_lds_kb=lds_kb):
        _check(dev, idx, reads, wants, (seed_fuse, lds_kb))
    dev.set_debug(True)


def _cell1_count(oi, q):
    """Anchors of q at reference positions from 32,768 on (cell 1 of its contig)."""
    a = oi.anchors(q, 10, 15, MID)[0]
    return int(np.count_nonzero((a[:, 0] & np.uint64(0x7fffffff)) >= np.uint64(1 << 15))) if len(a) else 0


@pytest.fixture(scope="module")
def seg_reads(world):
    """Per length L, a slice of the dense world's contig c2 (unique sequence
    there: an anchor per minimizer) from 3,000 bases before the cell edge at
    32,768 to the base at which cell 1 holds L anchors; cell 0 holds ~500."""
    oi, _, rseqs, _, contigs = world
    c2, edge = contigs[2], 1 << 15
    picked, have = [], set()
    for L in SEG_LENS:
        a, b = edge, edge + 2000
        while a < b:                          # first end with >= L anchors in cell 1
            m = (a + b) // 2
            if _cell1_count(oi, c2[edge - 3000:m]) < L:
                a = m + 1
            else:
                b = m
        q = c2[edge - 3000:a]
        if L in set(_seg_lengths(oi.anchors(q, 10, 15, MID)[0]).tolist()):
            picked.append(q)
            have.add(L)
    reads = picked + [rseqs[0], rseqs[8] + rseqs[16]]
    return reads, have, _wants(oi, reads)


@pytest.mark.parametrize("read_tiny", [16, 1])
def test_sort_rank_segments(dev, world, seg_reads, read_tiny):
    """Rank phase: kept cells of 1, 2, 16, 17, 64 and 65 keys, ranked by the
    linear scan up to read_tiny keys and by the chunk search beyond."""
    idx = world[1]
    reads, have, wants = seg_reads
    assert have >= set(SEG_LENS), f"segment lengths not found: {sorted(set(SEG_LENS) - have)}"
    with knobs(dev, sort_small=1, read_tiny=read_tiny):
        _check(dev, idx, reads, wants, ("read_tiny", read_tiny))
    dev.set_debug(True)
