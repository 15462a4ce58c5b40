"""The row-partitioned entry points the host double cannot run (include/pgh.h: pgh_dist_need_counts / _need_list / _set_send_lists / _pack /
_compact_from_dense, pgh_graph_set_gather_bases_split, pgh_dist_partial_stage 1 and 2, pgh_dist_watch_isolated / _release_isolated) called
directly on the GPU, every call against numpy or against another route of the same engine.  All slices of a partition live in this one
process; the exchange is done here, in numpy.  The dense gather layout and the loop's scalars: kernel_checks.check_partitioned_steps_against_numpy.

Shapes.  The LDS hot cache holds the first 29 696 slots of a column block, sources sort by descending entry count, so a block has cold slots
only when more than 29 696 of its sources have entries.  The smallest graphs that get there: two blocks of 32 750 sources with entries
(W = 2), four such blocks (W = 4) -- the last 6 108 / 12 216 ranks are sources with one to three entries, so every cold slot is wanted by
some slices and not by others -- plus 6 001 isolated ids (no multiple of 4) and 7 sink-only ids (they only pad the id space behind the
live slots: the engine knows the isolated tail of GENERATED partitions alone, so these ids reach no watch code); and two generated pairs,
rmat_partitioned(16, 8, r, 2) (16 815 sources with entries per block: no cold slot, no cold image, the isolated-row watch has nothing to
pass over) and rmat_partitioned(17, 8, r, 2) (32 093 per block: the smallest generated pair with a cold image, where the watch is live).
The cold image and the compact numbering are forced onto these small slices by the switches of test_row_partitioned_path_on_one_gpu,
set around the uploads only (pb_plan reads them per build)."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

from kernel_checks import DistState, EPS32, F32, _restore_env, relabelled, row_normalised

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
ALPHA = 0.85
FORCED_IMAGE = dict(PGH_PB="1", PGH_PB_FORCE="1", PGH_PB_HEAVY="64", PGH_PB_HUBMAX="500")
SWITCHES = tuple(FORCED_IMAGE) + ("PGH_DIST_NEED_LISTS", "PGH_BLOCKS")
HOT_PAD = 32768          # the hot cache's read-ahead behind a block's slice (pygrank_amd/distributed.py)


def _lib():
    from pygrank_amd import _lib as L
    return L, L.lib()


def f32(vec):
    return vec.numpy(F32)


def dev(a):
    from pygrank_amd.device import DeviceVector
    return DeviceVector.from_host(np.ascontiguousarray(a, dtype=F32))


def full(n, value):
    from pygrank_amd.device import DeviceVector
    return DeviceVector.full(n, value)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ptr(arr):
    return arr.ctypes.data_as(C.c_void_p)


def signed(rng, n):
    return (rng.random(n) * 4 - 2).astype(F32).astype(np.float64)


def _graph_with_cold_slots(seed, with_entries, few_entries):
    """with_entries sources of which the last few_entries have 1-3 entries (the others 4-10), 6 001 isolated ids, 7 sink-only ids; ids
    shuffled, real weights in [0.5, 2), rows normalised: the matrix a preprocessor would hand to partition_scipy."""
    rng = np.random.default_rng(seed)
    n = with_entries + 6001 + 7
    ids = rng.permutation(n)
    senders, sinks = ids[:with_entries], ids[with_entries:with_entries + 7]
    receivers = np.concatenate((senders, sinks))
    counts = np.concatenate((rng.integers(4, 11, with_entries - few_entries), rng.integers(1, 4, few_entries)))
    rows = np.repeat(senders, counts)
    cols = rng.choice(receivers, len(rows))
    rows, cols = np.concatenate((rows, senders[:21])), np.concatenate((cols, np.repeat(sinks, 3)))       # every sink is pointed at
    A = sp.csr_array((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    A.sum_duplicates()
    A.data = rng.uniform(0.5, 2.0, A.nnz)
    A.sort_indices()
    return row_normalised(A)


class Partition:
    """All W slices of one matrix (compact numbering forced), optionally their dense twins, and what the tests derive from both."""

    def __init__(self, M, world, dense_twins):
        from pygrank_amd.distributed import partition_scipy
        L, lib = _lib()
        self.M, self.world = M, world
        saved = {k: os.environ.get(k) for k in SWITCHES}
        try:
            for k in SWITCHES:
                os.environ.pop(k, None)
            os.environ.update(FORCED_IMAGE)
            self.slices = [partition_scipy(M, r, world) for r in range(world)]
            os.environ["PGH_DIST_NEED_LISTS"] = "0"
            self.dense = [partition_scipy(M, r, world) for r in range(world)] if dense_twins else []
        finally:
            _restore_env(saved)
        self.perm = self.slices[0].perm.astype(np.int64)
        self.n, self.n_pad, self.m = M.shape[0], self.slices[0].n, self.slices[0].n_local
        self.pad = self.perm < 0
        nb, blk, hot = C.c_int32(), C.c_int64(), C.c_int32()
        self.lives = np.zeros((world, 8), dtype=np.int32)
        self.counts = np.zeros((world, 8), dtype=np.int64)
        self.hots = []
        for r, s in enumerate(self.slices):
            L.check(lib.pgh_graph_gather_layout(s.graph._h, C.byref(nb), C.byref(blk), ptr(self.lives[r])))
            L.check(lib.pgh_graph_hot_prefix(s.graph._h, C.byref(hot)))
            L.check(lib.pgh_dist_need_counts(s.graph._h, ptr(self.counts[r])))
            self.hots.append(hot.value)
        self.nb, self.blk, self.hot = nb.value, blk.value, self.hots[0]
        self.formats = [s.graph.format() for s in self.slices]
        # ---- what the slices reference, from the relabelled COO
        Mn = sp.coo_array(relabelled(M, self.perm))
        self.expected = []                                              # [slice][block] -> sorted unique slot - hot
        for r in range(world):
            mine = (Mn.col >= r * self.m) & (Mn.col < (r + 1) * self.m)
            block, slot = Mn.row[mine] // self.blk, Mn.row[mine] % self.blk
            self.expected.append([np.unique(slot[(block == b) & (slot >= self.hot)] - self.hot).astype(np.uint32) for b in range(self.nb)])
        self.lists = None

    def establish(self):
        """The shape does what it is there for (a test that cannot establish this fails)."""
        where = (self.world, self.formats)
        assert self.nb == self.world and self.nb * self.blk == self.n_pad, where
        assert all(h == self.hot for h in self.hots) and self.hot > 0, (where, self.hots)                  # hot-only streams
        assert np.all(self.lives[:, :self.nb] > self.hot + 1000), (where, self.lives)
        assert np.all(self.counts[:, :self.nb] > 0), (where, self.counts)
        assert all("propagation-blocking" in fmt for fmt in self.formats), where
        for r in range(self.world):
            for b in range(self.nb):                                                                        # strict subsets of the live cold slots
                assert 0 < len(self.expected[r][b]) < self.lives[r, b] - self.hot, (where, r, b)
        assert any(not np.array_equal(self.expected[0][b], self.expected[1][b]) for b in range(self.nb)), where

    def need_lists(self):
        """[slice][block] as pgh_dist_need_list hands them out"""
        if self.lists is None:
            L, lib = _lib()
            self.lists = []
            for r, s in enumerate(self.slices):
                row = []
                for b in range(self.nb):
                    out = np.full(int(self.counts[r, b]), 0xFFFFFFFF, dtype=np.uint32)
                    L.check(lib.pgh_dist_need_list(s.graph._h, b, ptr(out)))
                    row.append(out)
                self.lists.append(row)
        return self.lists

    def register(self, owner, stretches):
        """pgh_dist_set_send_lists on slice `owner`: stretches = one array of slots per destination (destination-major; one local block)"""
        L, lib = _lib()
        slots = np.ascontiguousarray(np.concatenate(stretches) if stretches else np.zeros(0), dtype=np.uint32)
        offs = np.concatenate(([0], np.cumsum([len(s) for s in stretches]))).astype(np.int64)
        local = np.zeros(max(len(stretches), 1), dtype=np.int32)
        L.check(lib.pgh_dist_set_send_lists(self.slices[owner].graph._h, ptr(slots), ptr(local), ptr(offs), len(stretches)))
        return int(offs[-1])

    def split_bases(self, r):
        """[j][rank][hot] | [block][referenced cold slots], as _Buffers lays a compact slice's gather vector out (one block per rank)"""
        L, lib = _lib()
        hot_bases, cold_bases = np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64)
        prefix = np.concatenate(([0], np.cumsum(self.counts[r, :self.nb])))
        hot_bases[:self.nb] = np.arange(self.nb) * self.hot
        cold_bases[:self.nb] = self.nb * self.hot + prefix[:-1]
        L.check(lib.pgh_graph_set_gather_bases_split(self.slices[r].graph._h, ptr(hot_bases), ptr(cold_bases)))
        return hot_bases, cold_bases, int(self.nb * self.hot + prefix[-1] + HOT_PAD)

    def dense_bases(self, g):
        L, lib = _lib()
        bases = np.zeros(8, dtype=np.int64)
        bases[:self.nb] = np.arange(self.nb) * self.blk
        L.check(lib.pgh_graph_set_gather_bases(g._h, ptr(bases)))
        return bases


@pytest.fixture(scope="module")
def two(gpu_engine):
    return Partition(_graph_with_cold_slots(71, 65500, 12000), 2, dense_twins=True)


@pytest.fixture(scope="module")
def four(gpu_engine):
    return Partition(_graph_with_cold_slots(72, 131000, 24000), 4, dense_twins=False)


def test_need_lists_are_the_referenced_cold_slots(two, four):
    L, lib = _lib()
    for part in (two, four):
        part.establish()
        lists = part.need_lists()
        for r, s in enumerate(part.slices):
            for b in range(part.nb):
                got, want = lists[r][b], part.expected[r][b]
                assert np.all(np.diff(got.astype(np.int64)) > 0), (part.world, r, b, "not strictly ascending")
                assert np.array_equal(got, want), (part.world, r, b, len(got), len(want), part.formats[r])
                assert got[-1] == part.lives[r, b] - part.hot - 1, (part.world, r, b)
            # counts is [num_blocks] (include/pgh.h): the call writes exactly that many entries and leaves what lies behind them alone --
            # blocks >= num_blocks have no count to read; asking for their list is refused (test_refusals_name_themselves_and_write_nothing)
            counts = np.full(8, -1, dtype=np.int64)
            L.check(lib.pgh_dist_need_counts(s.graph._h, ptr(counts)))
            assert np.array_equal(counts[:part.nb], [len(x) for x in lists[r]]) and np.all(counts[part.nb:] == -1), (part.world, r, counts)
        for r, d in enumerate(part.dense):                              # PGH_DIST_NEED_LISTS=0: no list, every count zero
            counts = np.full(8, -1, dtype=np.int64)
            L.check(lib.pgh_dist_need_counts(d.graph._h, ptr(counts)))
            assert np.all(counts[:part.nb] == 0) and np.all(counts[part.nb:] == -1), (part.world, r, counts)


def test_pack_fills_every_stretch_with_the_requested_rows(two, four):
    L, lib = _lib()
    for part in (two, four):
        part.establish()
        lists, W, m, hot = part.need_lists(), part.world, part.m, part.hot
        index_valued = dev(np.arange(m))                                # row i holds float(i): exact below 2^24
        for owner in range(W):
            g = part.slices[owner].graph
            part.split_bases(owner)                                     # (slices stored by row)
            stretches = [lists[r][owner] for r in range(W)]
            if W == 4:
                stretches[1 + owner % 2] = np.zeros(0, dtype=np.uint32)     # a destination that asks for nothing, between two that do
            total = part.register(owner, stretches)
            want = np.concatenate([hot + s.astype(np.int64) for s in stretches]).astype(F32)
            assert total == len(want) and total > 0
            exact, longer, short = full(total, SENTINEL), full(total + 3, SENTINEL), full(total - 1, SENTINEL)
            L.check(lib.pgh_dist_pack(g._h, index_valued._h, exact._h))                 # a buffer exactly send_total long
            assert np.array_equal(f32(exact), want), (W, owner, np.flatnonzero(f32(exact) != want)[:5])
            L.check(lib.pgh_dist_pack(g._h, index_valued._h, longer._h))
            assert np.array_equal(f32(longer)[:total], want) and np.all(f32(longer)[total:] == SENTINEL), (W, owner)
            assert lib.pgh_dist_pack(g._h, index_valued._h, short._h) != 0 and b"pgh_dist_pack" in lib.pgh_last_error(), (W, owner)
            assert np.all(f32(short) == SENTINEL), (W, owner, "a refused pack wrote")
            # segments = 0: nothing registered, nothing packed
            assert part.register(owner, []) == 0
            untouched = full(total, SENTINEL)
            L.check(lib.pgh_dist_pack(g._h, index_valued._h, untouched._h))
            assert np.all(f32(untouched) == SENTINEL), (W, owner)
            # refused lists: a local block the slice does not have, decreasing offsets
            slots, offs = np.ascontiguousarray(stretches[0][:8]), np.array([0, 8], dtype=np.int64)
            beyond, before, first = np.array([1], dtype=np.int32), np.array([-1], dtype=np.int32), np.zeros(3, dtype=np.int32)
            assert lib.pgh_dist_set_send_lists(g._h, ptr(slots), ptr(beyond), ptr(offs), 1) != 0, (W, owner)
            assert b"pgh_dist_set_send_lists" in lib.pgh_last_error()
            assert lib.pgh_dist_set_send_lists(g._h, ptr(slots), ptr(before), ptr(offs), 1) != 0, (W, owner)
            bad = np.array([0, 6, 4, 8], dtype=np.int64)
            assert lib.pgh_dist_set_send_lists(g._h, ptr(slots), ptr(first), ptr(bad), 3) != 0, (W, owner)
            assert b"pgh_dist_set_send_lists" in lib.pgh_last_error()
            assert np.array_equal(slots, stretches[0][:8]) and np.array_equal(bad, [0, 6, 4, 8])


def test_compact_from_dense_equals_the_packed_stretch(two, four):
    L, lib = _lib()
    for part in (two, four):
        part.establish()
        lists, W, m, hot, blk = part.need_lists(), part.world, part.m, part.hot, part.blk
        index_valued = dev(np.arange(m))
        for owner in range(W):                                          # block `owner` is the owner's only local block
            part.split_bases(owner)
            total = part.register(owner, [lists[r][owner] for r in range(W)])
            packed = full(total, SENTINEL)
            L.check(lib.pgh_dist_pack(part.slices[owner].graph._h, index_valued._h, packed._h))
            packed = f32(packed)
            at = 0
            for r in range(W):
                count = len(lists[r][owner])
                # a dense copy of the block's cold part behind `dense_base` sentinels; the output behind `out_base` sentinels
                dense_base, out_base = 5 + 3 * r, 7 + r
                dense = np.full(dense_base + blk, SENTINEL, dtype=F32)
                dense[dense_base:dense_base + blk - hot] = np.arange(hot, blk)
                out, dense_dev = full(out_base + count + 9, SENTINEL), dev(dense)      # (named: a handle must outlive the call)
                L.check(lib.pgh_dist_compact_from_dense(part.slices[r].graph._h, owner, dense_dev._h, dense_base, out._h, out_base))
                got = f32(out)
                assert np.array_equal(got[out_base:out_base + count], packed[at:at + count]), (W, owner, r)
                assert np.all(got[:out_base] == SENTINEL) and np.all(got[out_base + count:] == SENTINEL), (W, owner, r, "wrote outside its stretch")
                at += count
            assert at == total


def _exchange(part, xg_slices):
    """The gather vector of every compact slice, three ways: (a) hot prefixes + the pack stretches of the owners, (b) hot prefixes + the
    slice's own compaction of a dense copy, (c) the dense layout of the twins.  xg_slices: every rank's slice, by row (numpy f32)."""
    L, lib = _lib()
    lists, W, nb, blk, hot = part.need_lists(), part.world, part.nb, part.blk, part.hot
    xg_all = np.concatenate(xg_slices).astype(F32)
    packed = []
    for owner in range(W):
        part.split_bases(owner)
        total = part.register(owner, [lists[r][owner] for r in range(W)])
        buf, mine = full(total, SENTINEL), dev(xg_slices[owner])
        L.check(lib.pgh_dist_pack(part.slices[owner].graph._h, mine._h, buf._h))
        edges = np.concatenate(([0], np.cumsum([len(lists[r][owner]) for r in range(W)])))
        packed.append([f32(buf)[edges[r]:edges[r + 1]] for r in range(W)])
    dense_dev = dev(xg_all)
    by_pack, by_compaction = [], []
    for r in range(W):
        hot_bases, cold_bases, length = part.split_bases(r)
        a = np.zeros(length, dtype=F32)
        for b in range(nb):
            a[hot_bases[b]:hot_bases[b] + hot] = xg_all[b * blk:b * blk + hot]
        b_vec = dev(a)
        for b in range(nb):
            a[cold_bases[b]:cold_bases[b] + len(lists[r][b])] = packed[b][r]
            L.check(lib.pgh_dist_compact_from_dense(part.slices[r].graph._h, b, dense_dev._h, b * blk + hot, b_vec._h, int(cold_bases[b])))
        by_pack.append(a)
        by_compaction.append(b_vec)
    dense = np.concatenate((xg_all, np.zeros(HOT_PAD, dtype=F32)))
    return by_pack, by_compaction, dense


def _step(g, xg_full, p, stages=None, poison=None):
    """one pgh_dist_partial (or its stages) + pgh_dist_combine from a fresh state -> (y, xg_local_out, d[2]) as bits.
    poison = (vector with NaN where stage 1 must not read, the real vector): stage 1 runs on the first, stage 2 on the second's values."""
    L, lib = _lib()
    state = DistState()
    m = len(p)
    y, xo = full(m, SENTINEL), full(m, SENTINEL)
    if poison is not None:
        bad, good = poison
        L.check(lib.pgh_dist_partial_stage(g._h, bad._h, state.ptr, 1))
        L.check(lib.pgh_sync())                                         # stage 1 has read what it reads; now the cold values arrive
        L.check(lib.pgh_vec_h2d_f32(bad._h, ptr(good), len(good)))
        L.check(lib.pgh_dist_partial_stage(g._h, bad._h, state.ptr, 2))
    elif stages is None:
        L.check(lib.pgh_dist_partial(g._h, xg_full._h, state.ptr))
    else:
        for stage in stages:
            L.check(lib.pgh_dist_partial_stage(g._h, xg_full._h, state.ptr, stage))
    L.check(lib.pgh_dist_combine(g._h, p._h, ALPHA, y._h, xo._h, state.ptr))
    return f32(y), f32(xo), state.read()[2]


def _operands(part, seed):
    """signed iterate and personalization (new ids, zero on padding ids), every rank's gather slice, and the f64 reference of one step"""
    L, lib = _lib()
    rng = np.random.default_rng(seed)
    x = np.where(part.pad, 0.0, signed(rng, part.n_pad))
    p = np.where(part.pad, 0.0, signed(rng, part.n_pad) * (rng.random(part.n_pad) < 0.5))
    m = part.m
    xg = []
    for r, s in enumerate(part.slices):
        out, mine = full(m, SENTINEL), dev(x[r * m:(r + 1) * m])
        L.check(lib.pgh_dist_prescale(s.graph._h, mine._h, out._h))
        xg.append(f32(out))
    Mn = relabelled(sp.csr_array(part.M.astype(F32).astype(np.float64)), part.perm)      # valued slices: the f32-rounded matrix
    ref = (1 - ALPHA) * p + ALPHA * (x @ Mn)
    bound = (1 - ALPHA) * np.abs(p) + ALPHA * (np.abs(x) @ abs(Mn))
    return x, p, xg, ref, bound


def test_layouts_agree(two):
    """(a) compact slice + pack stretches, (b) compact slice + its own compaction of a dense copy, (c) the dense twin: (a) and (b) are the
    same bits; (a) and (c) meet the bound of check_partitioned_steps_against_numpy (different images add in a different order)."""
    lib = _lib()[1]
    part = two
    part.establish()
    assert all("value-free" not in fmt for fmt in part.formats), part.formats        # uploads of a caller's matrix are valued: 4 EPS32
    x, p, xg, ref, bound = _operands(part, 5)
    by_pack, by_compaction, dense = _exchange(part, xg)
    m = part.m
    for r in range(part.world):
        g, twin = part.slices[r].graph, part.dense[r].graph
        pr = dev(p[r * m:(r + 1) * m])
        assert same_bits(f32(by_compaction[r]), by_pack[r]), (r, "the two exchanges fill the gather vector differently")
        part.split_bases(r)
        ya, xa, sa = _step(g, dev(by_pack[r]), pr)
        yb, xb, sb = _step(g, by_compaction[r], pr)
        assert same_bits(ya, yb) and same_bits(xa, xb) and sa == sb, (r, part.formats[r])
        part.dense_bases(twin)
        yc, xc, sc = _step(twin, dev(dense), pr)
        for label, y, s in (("compact", ya, sa), ("dense twin", yc, sc)):
            err = np.abs(y.astype(np.float64) - ref[r * m:(r + 1) * m])
            limit = 4 * EPS32 * bound[r * m:(r + 1) * m] + 1e-30                       # check_fused_steps' bound (valued slices)
            assert np.all(err <= limit), (r, label, float(np.max(err / np.maximum(limit, 1e-300))), part.formats[r])
            assert abs(s - y.astype(np.float64).sum()) <= 1e-12 * max(1.0, np.abs(y).sum()), (r, label)      # f64 sum of the returned y
            assert np.all(y[part.pad[r * m:(r + 1) * m]] == 0), (r, label, "padding ids")
        # ---- refusals that must leave the layout alone: the same step gives the same bits afterwards
        part.split_bases(r)
        bases = np.zeros(8, dtype=np.int64)
        assert lib.pgh_graph_set_gather_bases(g._h, ptr(bases)) != 0 and b"pgh_graph_set_gather_bases" in lib.pgh_last_error(), r      # compact slice
        hot_bases, cold_bases, _ = part.split_bases(r)
        far, moved = cold_bases.copy(), hot_bases + 64
        far[part.nb - 1] = 1 << 31
        assert lib.pgh_graph_set_gather_bases_split(g._h, ptr(moved), ptr(far)) != 0, r
        assert b"pgh_graph_set_gather_bases_split" in lib.pgh_last_error(), r
        assert same_bits(_step(g, dev(by_pack[r]), pr)[0], ya), (r, "a refused layout was applied in part")
        part.dense_bases(twin)
        far = np.zeros(8, dtype=np.int64)
        far[:part.nb] = 64 + np.arange(part.nb) * part.blk
        far[part.nb - 1] = 1 << 31
        assert lib.pgh_graph_set_gather_bases(twin._h, ptr(far)) != 0 and b"pgh_graph_set_gather_bases" in lib.pgh_last_error(), r
        assert same_bits(_step(twin, dev(dense), pr)[0], yc), (r, "a refused layout was applied in part")


def test_stages_are_the_whole_partial(two):
    """stage 1 then 2 == stage 0 == pgh_dist_partial; stage 1 reads nothing behind the hot prefixes: with the cold region full of NaN
    during stage 1 and the real values in place before stage 2, the step gives the same bits (the overlapped exchange rests on this)."""
    part = two
    part.establish()
    x, p, xg, ref, bound = _operands(part, 6)
    by_pack, _, dense = _exchange(part, xg)
    m, hot, blk, nb = part.m, part.hot, part.blk, part.nb
    L, lib = _lib()
    for r in range(part.world):
        pr = dev(p[r * m:(r + 1) * m])
        twin_hot = C.c_int32()
        L.check(lib.pgh_graph_hot_prefix(part.dense[r].graph._h, C.byref(twin_hot)))
        assert twin_hot.value == hot and "propagation-blocking" in part.dense[r].graph.format(), (r, twin_hot.value, part.dense[r].graph.format())
        for label, g, real in (("compact", part.slices[r].graph, by_pack[r]), ("dense twin", part.dense[r].graph, dense)):
            if label == "compact":
                part.split_bases(r)
                cold = np.zeros(len(real), dtype=bool)
                cold[nb * hot:] = True
            else:
                part.dense_bases(g)
                cold = np.zeros(len(real), dtype=bool)
                for b in range(nb):
                    cold[b * blk + hot:(b + 1) * blk] = True
            clean = _step(g, dev(real), pr)
            assert not np.any(np.isnan(clean[0])), (r, label)
            for stages in ((0,), (1, 2)):
                got = _step(g, dev(real), pr, stages=stages)
                assert same_bits(got[0], clean[0]) and same_bits(got[1], clean[1]) and got[2] == clean[2], (r, label, stages)
            poisoned = real.copy()
            poisoned[cold] = np.nan
            got = _step(g, None, pr, poison=(dev(poisoned), np.ascontiguousarray(real, dtype=F32)))
            assert same_bits(got[0], clean[0]) and same_bits(got[1], clean[1]) and got[2] == clean[2], (r, label, "stage 1 read a cold slot",
                                                                                                         int(np.isnan(got[0]).sum()))


# ---------------------------------------------------------------------------------------------------------------- isolated rows
class GeneratedPair:
    """rmat_partitioned(scale, 8, r, 2) with the cold image forced, the reference matrix (oracle/rmat_np, relabelled by perm) and where the
    isolated tail of every slice's block starts (ids without any edge sort last; the engine rounds the start up to whole float4s)."""

    def __init__(self, scale):
        from oracle import ref_loops as orc, rmat_np
        from pygrank_amd.distributed import rmat_partitioned
        L, lib = _lib()
        saved = {k: os.environ.get(k) for k in SWITCHES}
        try:
            for k in SWITCHES:
                os.environ.pop(k, None)
            os.environ.update(FORCED_IMAGE)
            self.slices = [rmat_partitioned(scale, 8, r, 2) for r in range(2)]
        finally:
            _restore_env(saved)
        self.formats = [s.graph.format() for s in self.slices]
        A = rmat_np.rmat_csr(scale, 8, seed=0)
        self.M = sp.csr_array(orc.normalize(A, "col", True))
        self.perm = self.slices[0].perm.astype(np.int64)
        self.n, self.m = A.shape[0], self.slices[0].n_local
        assert np.array_equal(np.sort(self.perm), np.arange(self.n)) and np.array_equal(self.slices[1].perm, self.perm)
        touched = (np.diff(A.indptr) > 0) | (np.bincount(A.indices, minlength=self.n) > 0)
        self.isolated_new = ~touched[self.perm]                          # by new id
        nb, blk = C.c_int32(), C.c_int64()
        L.check(lib.pgh_graph_gather_layout(self.slices[0].graph._h, C.byref(nb), C.byref(blk), None))
        assert nb.value == 2 and blk.value == self.m, (nb.value, blk.value)
        self.iso_begin = []
        for r in range(2):
            mine = self.isolated_new[r * self.m:(r + 1) * self.m]
            first = self.m - int(np.argmin(mine[::-1])) if not mine.all() else 0      # behind the last id with an edge
            assert mine[first:].all() and first < self.m, (scale, r)
            self.iso_begin.append((first + 3) // 4 * 4)
        self.Mn = relabelled(self.M, self.perm)


@pytest.fixture(scope="module")
def generated(gpu_engine):
    return {16: GeneratedPair(16), 17: GeneratedPair(17)}


def _loop(pair, r, p, y0, xg_fulls, sums, bracket, prefill=0.0, kind="ppr", operands=None):
    """Two PageRank iterations (or one absorb / poly step) on slice r, the peers' part of the exchange replayed from xg_fulls / sums.
    -> per step (y, xg_local_out, d[2], residual share d[1]) as bits"""
    L, lib = _lib()
    g, m = pair.slices[r].graph, pair.m
    state = DistState()
    dp, prev = dev(p), dev(y0)
    if bracket:
        L.check(lib.pgh_dist_watch_isolated(g._h, dp._h, prev._h))
    out = []
    try:
        for it in range(len(xg_fulls)):
            L.check(lib.pgh_dist_partial(g._h, xg_fulls[it]._h, state.ptr))
            y, xo = full(m, prefill), full(m, prefill)
            if kind == "ppr":
                L.check(lib.pgh_dist_combine(g._h, dp._h, ALPHA, y._h, xo._h, state.ptr))
            elif kind == "absorb":
                L.check(lib.pgh_dist_combine_absorb(g._h, dp._h, operands[0]._h, operands[1]._h, y._h, xo._h, state.ptr))
            else:
                result = dev(operands[0])
                L.check(lib.pgh_dist_combine_poly(g._h, prev._h, y._h, 2.0, -1.0, result._h, -0.5, 0, xo._h, state.ptr))
            d2 = state.read()[2]
            if kind == "poly":
                out.append((f32(y), f32(xo), d2, state.read()[1], f32(result)))
                break
            state.set(2, sums[it])
            L.check(lib.pgh_dist_close_sum(state.ptr, 1))
            L.check(lib.pgh_dist_residual(L.ERR_L1, y._h, prev._h, state.ptr))
            out.append((f32(y), f32(xo), d2, state.read()[1]))
            prev = y
    finally:
        if bracket:
            L.check(lib.pgh_dist_release_isolated(g._h))
    return out


def _same_run(a, b):
    return len(a) == len(b) and all(same_bits(u[0], v[0]) and same_bits(u[1], v[1]) and u[2] == v[2] and u[3] == v[3] and
                                    (len(u) < 5 or same_bits(u[4], v[4])) for u, v in zip(a, b))


@pytest.mark.parametrize("scale", [16, 17])
def test_isolated_rows_are_passed_over_only_while_their_operands_are_zero(generated, scale):
    L, lib = _lib()
    pair = generated[scale]
    m, n = pair.m, pair.n
    live_image = scale == 17
    # the shape does what it is there for: scale 17 has sources behind the hot prefix, hence a cold image, hence a live watch
    assert all(("propagation-blocking" in fmt) == live_image for fmt in pair.formats), pair.formats
    assert all(0 < b < m - 1000 for b in pair.iso_begin), pair.iso_begin
    rng = np.random.default_rng(scale)
    quiet = ~pair.isolated_new
    x = np.where(quiet, signed(rng, n), 0.0)                            # zero on every isolated row
    p = np.where(quiet & (rng.random(n) < 0.5), signed(rng, n), 0.0)
    # ---- layouts: a slice with a cold image numbers its cold sources compactly (two regions, the cold one filled by the slice's own
    # compaction of a dense copy); without one the dense layout
    layouts = []
    for r, s in enumerate(pair.slices):
        counts, hot = np.zeros(8, dtype=np.int64), C.c_int32()
        L.check(lib.pgh_dist_need_counts(s.graph._h, ptr(counts)))
        L.check(lib.pgh_graph_hot_prefix(s.graph._h, C.byref(hot)))
        hot_bases, cold_bases = np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64)
        if counts.sum() > 0:
            prefix = np.concatenate(([0], np.cumsum(counts[:2])))
            hot_bases[:2], cold_bases[:2] = np.arange(2) * hot.value, 2 * hot.value + prefix[:-1]
            L.check(lib.pgh_graph_set_gather_bases_split(s.graph._h, ptr(hot_bases), ptr(cold_bases)))
            layouts.append((hot.value, hot_bases, cold_bases, counts, int(2 * hot.value + prefix[-1] + HOT_PAD)))
        else:
            hot_bases[:2] = np.arange(2) * m
            L.check(lib.pgh_graph_set_gather_bases(s.graph._h, ptr(hot_bases)))
            layouts.append(None)
    assert all((layout is not None) == live_image for layout in layouts), (scale, pair.formats)

    def exchange(y_slices):
        """every slice's gather vector from the iterates' slices"""
        xg = []
        for r, s in enumerate(pair.slices):
            out, mine = full(m, SENTINEL), dev(y_slices[r])
            L.check(lib.pgh_dist_prescale(s.graph._h, mine._h, out._h))
            xg.append(f32(out))
        xg_all = np.concatenate(xg)
        dense_dev = dev(np.concatenate((xg_all, np.zeros(HOT_PAD, dtype=F32))))
        vectors = []
        for r, s in enumerate(pair.slices):
            if layouts[r] is None:
                vectors.append(dense_dev)
                continue
            hot, hot_bases, cold_bases, counts, length = layouts[r]
            a = np.zeros(length, dtype=F32)
            for b in range(2):
                a[hot_bases[b]:hot_bases[b] + hot] = xg_all[b * m:b * m + hot]
            vec = dev(a)
            for b in range(2):
                L.check(lib.pgh_dist_compact_from_dense(s.graph._h, b, dense_dev._h, b * m + hot, vec._h, int(cold_bases[b])))
            vectors.append(vec)
        return vectors

    def unbracketed(p_all, x_all):
        """both slices, two iterations, the exchange and the all-reduce done here -> per slice: the run, and what a replay needs"""
        xg_fulls, sums, runs = [exchange([x_all[:m], x_all[m:]])], [], [[], []]
        states = [DistState(), DistState()]
        prev = [dev(x_all[:m]), dev(x_all[m:])]
        p_dev = [dev(p_all[:m]), dev(p_all[m:])]
        for it in range(2):
            ys, d2 = [], []
            for r, s in enumerate(pair.slices):
                L.check(lib.pgh_dist_partial(s.graph._h, xg_fulls[it][r]._h, states[r].ptr))
                y, xo = full(m, SENTINEL), full(m, SENTINEL)            # no watch: every row is written
                L.check(lib.pgh_dist_combine(s.graph._h, p_dev[r]._h, ALPHA, y._h, xo._h, states[r].ptr))
                ys.append(y)
                d2.append(states[r].read()[2])
                runs[r].append([f32(y), f32(xo), d2[-1], None])
            sums.append(float(np.sum(d2)))
            for r in range(2):
                states[r].set(2, sums[-1])
                L.check(lib.pgh_dist_close_sum(states[r].ptr, 1))
                L.check(lib.pgh_dist_residual(L.ERR_L1, ys[r]._h, prev[r]._h, states[r].ptr))
                runs[r][-1][3] = states[r].read()[1]
            prev = ys
            xg_fulls.append(exchange([f32(y) for y in ys]))
        return xg_fulls[:2], sums, runs

    xg_fulls, sums, plain = unbracketed(p, x)
    # the first step against numpy: value-free slices, check_partitioned_steps_against_numpy's bound with its one more EPS32
    ref = (1 - ALPHA) * p + ALPHA * (x @ pair.Mn)
    bound = 5 * EPS32 * ((1 - ALPHA) * np.abs(p) + ALPHA * (np.abs(x) @ abs(pair.Mn))) + 1e-30
    for r in range(2):
        assert "value-free" in pair.formats[r], pair.formats
        y1 = plain[r][0][0].astype(np.float64)
        assert np.all(np.abs(y1 - ref[r * m:(r + 1) * m]) <= bound[r * m:(r + 1) * m]), (scale, r)
        assert not np.any(plain[r][0][0] == SENTINEL) and np.all(y1[pair.isolated_new[r * m:(r + 1) * m]] == 0), (scale, r)
    for r in range(2):
        pr, xr, iso = p[r * m:(r + 1) * m], x[r * m:(r + 1) * m], pair.isolated_new[r * m:(r + 1) * m]
        tail = np.arange(m) >= pair.iso_begin[r]
        mine_full = [v[r] for v in xg_fulls]
        # ---- operands zero on every isolated row: which rows does a bracketed step leave alone?
        marked = _loop(pair, r, pr, xr, mine_full[:1], sums[:1], bracket=True, prefill=SENTINEL)[0][0]
        skipped = marked == SENTINEL
        assert not np.any(skipped & ~tail), (scale, r, "a row in front of the isolated tail was passed over")
        assert bool(skipped.any()) == live_image, (scale, r, int(skipped.sum()), pair.formats[r])
        run = _loop(pair, r, pr, xr, mine_full, sums, bracket=True)      # both iterate buffers hold zeros there, as the loops keep them
        assert all(np.all(step[0][iso] == 0) for step in run), (scale, r)
        assert _same_run(run, plain[r]), (scale, r, "bracketed != unbracketed", [(u[2], v[2], u[3], v[3]) for u, v in zip(run, plain[r])])
        # ---- after release an unbracketed step processes every row again
        again = _loop(pair, r, pr, xr, mine_full[:1], sums[:1], bracket=False, prefill=SENTINEL)[0]
        assert not np.any(again[0] == SENTINEL) and same_bits(again[0], plain[r][0][0]), (scale, r)
        # ---- p, or only the start iterate, non-zero on ONE isolated row: every row is processed, that row included
        for row in (pair.iso_begin[r], m - 1):
            assert iso[row]
            for which in ("p", "start"):
                p2, x2 = p.copy(), x.copy()
                (p2 if which == "p" else x2)[r * m + row] = 0.625
                fulls2, sums2, plain2 = unbracketed(p2, x2)
                run2 = _loop(pair, r, p2[r * m:(r + 1) * m], x2[r * m:(r + 1) * m], [v[r] for v in fulls2], sums2, bracket=True, prefill=SENTINEL)
                assert not np.any(run2[0][0] == SENTINEL), (scale, r, row, which, "rows passed over although an operand is non-zero")
                assert _same_run(run2, plain2[r]), (scale, r, row, which)
                if which == "p":                                        # (1 - alpha) p on a row without entries
                    assert abs(run2[0][0][row] - (1 - ALPHA) * 0.625) <= 4 * EPS32 * (1 - ALPHA) * 0.625, (scale, r, row, run2[0][0][row])
        # ---- one absorb and one poly step, bracketed and not
        deg, lam = (rng.random(m) + 0.1).astype(F32), (rng.random(m) + 0.1).astype(F32)
        res0 = np.where(quiet[r * m:(r + 1) * m], signed(rng, m), 0.0).astype(F32)
        for kind, operands in (("absorb", (dev(deg), dev(lam))), ("poly", (res0,))):
            base = _loop(pair, r, pr, xr, mine_full[:1], sums[:1], bracket=False, kind=kind, operands=operands)
            watched = _loop(pair, r, pr, xr, mine_full[:1], sums[:1], bracket=True, kind=kind, operands=operands)
            assert np.all(watched[0][0][iso] == 0), (scale, r, kind)
            assert _same_run(watched, base), (scale, r, kind, "bracketed != unbracketed")
            for row in (pair.iso_begin[r], m - 1):
                p2, x2 = pr.copy(), xr.copy()
                (p2 if kind == "absorb" else x2)[row] = 0.625           # absorb: p; poly: the term itself
                base = _loop(pair, r, p2, x2, mine_full[:1], sums[:1], bracket=False, prefill=SENTINEL, kind=kind, operands=operands)
                watched = _loop(pair, r, p2, x2, mine_full[:1], sums[:1], bracket=True, prefill=SENTINEL, kind=kind, operands=operands)
                assert not np.any(watched[0][0] == SENTINEL) and _same_run(watched, base), (scale, r, kind, row, "one non-zero isolated row")


def test_refusals_name_themselves_and_write_nothing(two):
    from pygrank_amd.distributed import partition_scipy
    from kernel_checks import partition_test_graph
    L, lib = _lib()
    part = two
    part.establish()
    compact, twin = part.slices[0].graph, part.dense[0].graph
    nb = part.nb

    def refused(rc, who):
        assert rc != 0 and who in lib.pgh_last_error(), (who, rc, lib.pgh_last_error())

    # ---- a tiny partition: its stream is not hot-only, the gather vector cannot be split
    rng = np.random.default_rng(9)
    tiny = partition_scipy(row_normalised(partition_test_graph(rng, 1501)[0]), 0, 2)
    zeros = np.zeros(8, dtype=np.int64)
    refused(lib.pgh_graph_set_gather_bases_split(tiny.graph._h, ptr(zeros), ptr(zeros)), b"pgh_graph_set_gather_bases_split")
    # ---- need lists: a block out of range, a slice without lists
    out = np.full(16, 0xFFFFFFFF, dtype=np.uint32)
    for g, block in ((compact, -1), (compact, nb), (twin, 0), (tiny.graph, 0)):
        refused(lib.pgh_dist_need_list(g._h, block, ptr(out)), b"pgh_dist_need_list")
    assert np.all(out == 0xFFFFFFFF)
    dense, target = full(part.blk + 8, 1.0), full(int(part.counts[0].max()) + 8, SENTINEL)
    for g, block in ((compact, -1), (compact, nb), (twin, 0), (tiny.graph, 0)):
        refused(lib.pgh_dist_compact_from_dense(g._h, block, dense._h, 0, target._h, 0), b"pgh_dist_compact_from_dense")
    short = full(int(part.counts[0, 0]) - 1, SENTINEL)                   # an output one element short
    refused(lib.pgh_dist_compact_from_dense(compact._h, 0, dense._h, 0, short._h, 0), b"pgh_dist_compact_from_dense")
    refused(lib.pgh_dist_compact_from_dense(compact._h, 0, dense._h, 0, target._h, -1), b"pgh_dist_compact_from_dense")
    assert np.all(f32(target) == SENTINEL) and np.all(f32(short) == SENTINEL) and np.all(f32(dense) == 1.0)
