"""
No result depends on what an earlier call left behind (needs a real MI355X: `pytest -m gpu`).  Bit-exact against oracle/c_oracle
and the host restatements, like test_gpu_parity.py; what varies here is the state a kernel starts from:

  * WORKSPACE: every gf2_ws_reserve site (DESIGN.md "State between calls") runs on a context of its own whose workspace slots are
    set to 0xFF and to 0x00 between identical calls (gf2_ctx_fill_workspace), once after a larger call has grown them;
  * OUTPUTS: every device output goes into a window of a parent filled with 0xA5.. (tests/state_check.py): promised words equal the
    reference, guards untouched, pitch padding as include/gf2hip.h says per entry point;
  * ACCUMULATION: histograms are added to bins that hold a non-zero ramp, twice;
  * ALIGNMENT: where a kernel picks a 16-byte path by the pointer, the same cases run with the window 8 bytes further on.
"""
import functools

import numpy as np
import pytest

from oracle import c_oracle
from quantum_css_codes_amd import _native, circuit_noise, ft_noise, stream_noise
from quantum_css_codes_amd.css_code import CSSCode
from quantum_css_codes_amd.montecarlo import dense_table, packed_word
from tests import stream_ref
from tests.state_check import DirtyBuffer, Layout, dirty_input, ramp

pytestmark = pytest.mark.gpu

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
OFFSETS = [(256, 256), (264, 256), (256, 264), (264, 264)]               # (errors, syndromes): byte offset of the window in its parent
OFFSET_IDS = ["aligned", "errors+8", "syndromes+8", "both+8"]


@pytest.fixture(scope="module")
def ctx():
    return _native.default_context()


@pytest.fixture
def route():
    context = _native.default_context()
    yield context
    context.set_flags(0)


@pytest.fixture
def fresh():
    """A context of its own (fresh workspace slots), closed at the end of the case."""
    context = _native.Context(0)
    yield context
    context.close()


def out(ctx, rows, pitch, lead=256, prefill=None):
    return DirtyBuffer(ctx, Layout(rows, pitch, lead), prefill)


def standard_check(rng, r, n, ioff):
    hm = rng.integers(0, 2, (r, n))
    if ioff is not None:
        hm[:, ioff:ioff + r] = np.identity(r, dtype=int)
    return _native.pack_rows(hm)


def workspace_sequence(context, slots, first, larger, grows=True):
    """first(): the call, compared with its reference; larger(): a larger call of the same route.  `slots`: the workspace slots
    the route carves up -- a non-zero size after the first call proves that the case reached its reserve site.  grows=False: a
    route whose workspace does not depend on the count (the histograms alone, or chunks of a fixed size)."""
    first()
    sizes = context.fill_workspace(0xFF)
    assert all(sizes[s] > 0 for s in slots), (slots, sizes)
    first()
    larger()
    grown = context.fill_workspace(0x00)
    assert all(g >= s for g, s in zip(grown, sizes)) and any(g > s for g, s in zip(grown, sizes)) == grows, (sizes, grown)
    first()


def test_fill_workspace_arguments(fresh):
    assert fresh.fill_workspace(0) == [0, 0, 0, 0]
    for bad in (-1, 256):
        with pytest.raises(_native.GF2Error, match="outside 0..255"):
            fresh.fill_workspace(bad)
    assert _native.lib().gf2_ctx_fill_workspace(fresh.handle, 0xFF, None) == _native.GF2_OK


# ---- workspace: gf2_syndrome_dev, gf2_syndrome_sparse_dev ------------------------------------------------------------------------

@pytest.mark.parametrize("batch", [100, 65])
def test_workspace_syndrome_dev_sample_major(fresh, batch):
    # slot 1: the tiled copy of the errors and the slab-major syndromes; 100 and 65 samples leave pad samples in the last tile
    r, n = 130, 300
    rng = np.random.default_rng(batch)
    h = _native.pack_rows(rng.integers(0, 2, (r, n)))
    chk = fresh.check_create(h, r, n)

    e = _native.pack_rows(rng.integers(0, 2, (batch, n)))
    big = _native.pack_rows(rng.integers(0, 2, (1000, n)))
    e_buf, big_buf = fresh.alloc(e.nbytes).upload(e), fresh.alloc(big.nbytes).upload(big)
    want = c_oracle.syndrome_batch(h, r, n, e, batch)

    def run(buf, count):
        s = out(fresh, count, chk.slabs + 1)
        fresh.syndrome_dev(chk, buf, count, e.shape[1], s.view, chk.slabs + 1)
        return s

    workspace_sequence(fresh, [1], lambda: run(e_buf, batch).check(want, preserved=True, what="syndromes"), lambda: run(big_buf, 1000))


@pytest.mark.parametrize("stored", [False, True], ids=["histogram", "syndromes+histogram"])
@pytest.mark.parametrize("case", [(100, 300, 100, 130, 0.05, None), (2047, 4096, 2048, 1500, 0.007, None),
                                  (100, 300, 100, 9000, 0.05, 12), (1023, 2048, 1024, 9000, 0.01, 12)],
                         ids=["100x300", "2047x4096", "three-passes", "three-passes-hand-scheduled"])
def test_workspace_sparse_slabs(fresh, case, stored):
    # slot 2: records, partial weights (two passes' worth), redo counter and list, the syndrome sink
    r, n, ioff, batch, density, pass_log2 = case
    rng = np.random.default_rng(r + batch)
    h = standard_check(rng, r, n, ioff)
    chk = fresh.check_create(h, r, n)
    fresh.set_flags(_native.F_SPARSE_SLABS)
    if pass_log2:
        fresh.set_option(_native.OPT_SLAB_PASS_LOG2, pass_log2)
    e = _native.pack_rows((rng.random((batch, n)) < density).astype(np.uint8))
    big = _native.pack_rows((rng.random((3 * batch, n)) < density).astype(np.uint8))
    e_buf, big_buf = fresh.alloc(e.nbytes).upload(e), fresh.alloc(big.nbytes).upload(big)
    want_s = c_oracle.syndrome_batch(h, r, n, e, batch)
    want_h = c_oracle.histogram(want_s, batch, r, 1, r + 1)
    lds = want_s.shape[1]

    def run(buf, count):
        hist = out(fresh, 1, r + 1, prefill=ramp(r + 1))
        s = out(fresh, count, lds) if stored else None
        fresh.syndrome_sparse_dev(chk, buf, count, e.shape[1], s.view if stored else None, lds if stored else 0, hist.view, r + 1)
        return s, hist

    def first():
        s, hist = run(e_buf, batch)
        hist.check_accumulated(ramp(r + 1), want_h)
        if stored:
            s.check(want_s, what="syndromes")

    workspace_sequence(fresh, [2], first, lambda: run(big_buf, 3 * batch))


# ---- workspace: gf2_mc_run, gf2_mc_decode, gf2_mc_circuit_run ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mc_shape(name):
    """(h1, r1, h2, r2, n) of the three Monte-Carlo shapes; computed once, never modified."""
    if name == "steane":
        h = c_oracle.pack_rows(STEANE)
        return h, 3, h, 3, 7
    n, r1, r2, off2 = {"lane": (127, 63, 64, 63), "records": (1023, 511, 511, 512)}[name]
    rng = np.random.default_rng(n + r1)
    hm1, hm2 = rng.integers(0, 2, (r1, n)), rng.integers(0, 2, (r2, n))
    hm1[:, :r1] = np.identity(r1, dtype=int)
    hm2[:, off2:off2 + r2] = np.identity(r2, dtype=int)
    return _native.pack_rows(hm1), r1, _native.pack_rows(hm2), r2, n


MC_ARGS = {"steane": (0xC55, 77, 0.04, 0.01, 0.02, _native.HIST_FULL), "lane": (77, 1000, 0.004, 0.003, 0.005, _native.HIST_WEIGHT),
           "records": (31, 500, 0.01, 0.005, 0.005, _native.HIST_WEIGHT)}


@functools.lru_cache(maxsize=None)
def mc_reference(name, count):
    h1, r1, h2, r2, n = mc_shape(name)
    seed, first, p_x, p_y, p_z, mode = MC_ARGS[name]
    want = c_oracle.mc(h1, r1, h2, r2, n, seed, first, count, p_x, p_y, p_z, 0 if mode == _native.HIST_FULL else 1)
    for w in want:
        w.setflags(write=False)
    return want


#            shape, routing flag, the workspace slots the route carves up, whether they grow with the count
MC_ROUTES = {"fused-small-code": ("steane", None, [0], False), "lane-kernel": ("lane", None, [0], True),
             "record-sampler": ("records", None, [0, 2, 3], True), "GF2_MC_ROWS": ("records", "MC_ROWS", [0, 2, 3], False),
             "GF2_MC_FUSED": ("records", "MC_FUSED", [0], False), "GF2_MC_UNFUSED": ("records", "MC_UNFUSED", [0, 2], True),
             "GF2_MC_DENSE": ("records", "MC_DENSE", [0], True)}


@pytest.mark.parametrize("name", sorted(MC_ROUTES))
def test_workspace_mc_run(fresh, name):
    # slot 0: sampled errors (packed rows, or records + identity words + misfit lists), syndromes, the two histograms; slots 2 and
    # 3: the slab pipelines of the two components.  70001 samples take the route, 3000 its small-count neighbour on the same slots.
    shape, flag, slots, grows = MC_ROUTES[name]
    h1, r1, h2, r2, n = mc_shape(shape)
    c1, c2 = fresh.check_create(h1, r1, n), fresh.check_create(h2, r2, n)
    if flag:
        fresh.set_flags(getattr(_native, "F_" + flag))
    seed, first_sample, p_x, p_y, p_z, mode = MC_ARGS[shape]

    def run(count):
        return fresh.mc_run(c1, c2, seed, first_sample, count, p_x, p_y, p_z, mode)

    def first():
        for count in (70001, 3000):
            got, want = run(count), mc_reference(shape, count)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), count
            assert int(got[0].sum()) == count == int(got[1].sum())

    workspace_sequence(fresh, slots, first, lambda: run(150001), grows)


def test_workspace_mc_decode_and_circuit_run(fresh):
    # slot 0: gf2_mc_decode's two dense tables and five counters; gf2_mc_circuit_run's two histograms
    code = CSSCode(STEANE, STEANE)
    h1, h2 = c_oracle.pack_rows(code.parity_check_c1), c_oracle.pack_rows(code.parity_check_c2)
    t1, t2 = dense_table(code._c1_syndromes, 3, 7), dense_table(code._c2_syndromes, 3, 7)
    xop, zop = packed_word(code.x_operator_matrix()[0]), packed_word(code.z_operator_matrix()[0])
    c1, c2 = fresh.check_create(h1, 3, 7), fresh.check_create(h2, 3, 7)
    p = (0.03, 0.01, 0.02)
    want_d = c_oracle.mc_decode(h1, 3, h2, 3, 7, t1, t2, xop, zop, 77, 10**9, 50000, *p)
    idle = circuit_noise.FaultCircuit.for_code(code, [(_native.GATE_IDLE, q, 0) for q in range(7)])
    circ = fresh.circuit_create(idle.effects)
    want_z, want_x = c_oracle.mc(h1, 3, h2, 3, 7, 7, 5, 50000, *p, 0)       # a circuit of IDLE gates is the code-capacity model

    def first():
        got = fresh.mc_decode(c1, c2, t1, t2, xop, zop, 77, 10**9, 50000, *p)
        assert [int(v) for v in got] == [int(v) for v in want_d]
        hz, hx = fresh.mc_circuit_run(circ, 3, 3, 7, 5, 50000, *p, _native.HIST_FULL)
        assert np.array_equal(hz, want_z) and np.array_equal(hx, want_x)

    def larger():
        # (the slot grows with the bins: the weight mode of a 40-row layout is not larger, the full histograms of r = 12 are)
        wide = _native.pack_rows(np.random.default_rng(5).integers(0, 2, (12, 40)))
        w1, w2 = fresh.check_create(wide, 12, 40), fresh.check_create(wide, 12, 40)
        fresh.mc_run(w1, w2, 1, 0, 1000, *p, _native.HIST_FULL)

    workspace_sequence(fresh, [0], first, larger)


# ---- workspace: RREF and normalisation -------------------------------------------------------------------------------------------

#             m, n, batch, (option, value) or None, routing flag or None
RREF_SITES = {"small-matrix-batch": (129, 65, 33, None, None),                      # no workspace at all: rows in registers
              "sweeps-K2": (300, 2500, 3, (_native.OPT_RREF_SWEEP_K, 2), None),
              "sweeps-K4": (300, 2500, 3, (_native.OPT_RREF_SWEEP_K, 4), None),
              "pivot-rows-in-place": (300, 600, 400, None, None),
              "pair-kernels": (300, 2500, 3, (_native.OPT_RREF_SWEEP_K, 0), None),
              "streamed-one-chunk": (4100, 700, 2, None, None),                      # (16 words or fewer per row: nothing to look ahead to)
              "streamed-look-ahead": (4100, 1100, 2, None, None),
              "streamed-no-look-ahead": (4100, 1100, 2, None, "RREF_NO_LOOKAHEAD")}


@functools.lru_cache(maxsize=None)
def rref_reference(m, n, batch):
    rng = np.random.default_rng(m * 3 + n)
    mats = []
    for b in range(batch):
        a = (rng.random((m, n)) < (0.5 if b % 3 != 1 else 0.05)).astype(np.uint8)
        if m > 4:
            a[3] = a[0] ^ a[1]
            a[:, n // 2] = 0
        mats.append(_native.pack_rows(a))
    packed = np.ascontiguousarray(np.stack(mats))
    want = [c_oracle.rref(packed[b], m, n) for b in range(batch)]
    packed.setflags(write=False)
    return packed, want


def rref_dirty(context, packed, want, m, n, lead=256, with_pivots=True):
    """gf2_rref_batch_dev on a dirty copy of `packed`, with dirty pivots and ranks; compared with the oracle's `want`."""
    batch, ld, cap = packed.shape[0], packed.shape[2], min(m, n)
    a_view, a_buf = dirty_input(context, packed, lead)
    piv = out(context, batch, cap)
    rank = out(context, 1, batch)
    _native.check(_native.lib().gf2_rref_batch_dev(context.handle, a_view.ptr, batch, m, n, ld, piv.view.ptr if with_pivots else None,
                                                   rank.view.ptr))
    if want is None:
        return
    got = a_buf.layout.payload(a_buf.fetch(), "matrices").reshape(batch, m, ld)
    ranks = rank.check(np.array([[w[2] for w in want]], dtype=np.uint64), what="ranks")
    full = np.zeros((batch, cap), dtype=np.uint64)
    promised = np.zeros((batch, cap), dtype=bool)
    for b in range(batch):
        assert np.array_equal(got[b], want[b][0]), "matrix %d" % b
        full[b, :want[b][2]] = want[b][1]
        promised[b, :want[b][2]] = with_pivots                           # entries past the rank are left open by the header
    piv.check(full, promised=promised, preserved=not with_pivots, what="pivots")
    assert [int(v) for v in ranks[0]] == [w[2] for w in want]


@pytest.mark.parametrize("site", sorted(RREF_SITES))
def test_workspace_rref(fresh, site):
    # slot 1: the copy of the batch, pivot-row lists, states and used flags (memset per call), coefficients, snapshots, the side
    # buffer of column words (and, streamed, slots / tables / published words and two sets of them)
    m, n, batch, option, flag = RREF_SITES[site]
    if option:
        fresh.set_option(*option)
    if flag:
        fresh.set_flags(getattr(_native, "F_" + flag))
    packed, want = rref_reference(m, n, batch)
    ones = np.full_like(packed, 0xFFFFFFFFFFFFFFFF)
    if n % 64:
        ones[:, :, -1] = np.uint64((1 << (n % 64)) - 1)                  # (pad bits are zero on input)

    def first():
        rref_dirty(fresh, packed, want, m, n)

    if site == "small-matrix-batch":
        first()
        assert fresh.fill_workspace(0xFF) == [0, 0, 0, 0]                # the register kernels reserve nothing: nothing to dirty
        first()
        return
    first()
    sizes = fresh.fill_workspace(0xFF)
    assert sizes[1] > 0, sizes
    first()
    rref_dirty(fresh, ones, None, m, n)                                  # an all-ones batch of the same shape: rank 1, other states
    assert fresh.fill_workspace(0x00)[1] == sizes[1]
    first()


def test_workspace_and_outputs_normalize(fresh):
    # slot 1: the state (memset per call), the panel's coefficients and pivot-row snapshot; swaps, count and status dirty
    r, n, offset = 130, 300, 64
    rng = np.random.default_rng(130)
    while True:
        hm = rng.integers(0, 2, (r, n))
        rc, want_h, want_swaps = c_oracle.normalize(_native.pack_rows(hm), r, n, offset)
        if rc == 0:
            break
    h = _native.pack_rows(hm)

    def first():
        h_view, h_buf = dirty_input(fresh, h)
        swaps, count, status = out(fresh, 1, 2 * r), out(fresh, 1, 1), out(fresh, 1, 1)
        _native.check(_native.lib().gf2_normalize_dev(fresh.handle, h_view.ptr, r, n, h.shape[1], offset, swaps.view.ptr, count.view.ptr,
                                                      status.view.ptr))
        assert np.array_equal(h_buf.layout.payload(h_buf.fetch()).reshape(h.shape), want_h)
        count.check(np.array([[len(want_swaps)]], dtype=np.uint64), what="swap count")
        # (status is one int: the low half of its word is 0 = ok, the high half is left as it was)
        status.check(np.array([[0xA5A5A5A500000000]], dtype=np.uint64), what="status")
        full = np.zeros((1, 2 * r), dtype=np.uint64)
        flat = np.array(want_swaps, dtype=np.uint64).reshape(-1)
        full[0, :flat.size] = flat
        swaps.check(full, promised=np.arange(2 * r)[None, :] < flat.size, what="swaps")

    def larger():
        big = _native.pack_rows(np.identity(700, dtype=int)[:, ::-1])     # every step needs a column swap
        b_view, _ = dirty_input(fresh, big)
        swaps, count, status = out(fresh, 1, 1400), out(fresh, 1, 1), out(fresh, 1, 1)
        _native.check(_native.lib().gf2_normalize_dev(fresh.handle, b_view.ptr, 700, 700, big.shape[1], 0, swaps.view.ptr, count.view.ptr,
                                                      status.view.ptr))

    workspace_sequence(fresh, [1], first, larger)


# ---- outputs: gf2_syndrome_dev in each layout -----------------------------------------------------------------------------------

@pytest.mark.parametrize("offsets", OFFSETS, ids=OFFSET_IDS)
@pytest.mark.parametrize("shape", [(3, 7), (64, 64)])
def test_outputs_syndrome_small_sample_major(ctx, shape, offsets):
    # one word per sample on both sides and 16-byte aligned pointers: two samples per lane; any other pitch or address: one
    r, n = shape
    rng = np.random.default_rng(r)
    h = _native.pack_rows(rng.integers(0, 2, (r, n)))
    chk = ctx.check_create(h, r, n)
    for batch in (1, 2, 255, 513):
        bits = rng.integers(0, 2, (batch, n))
        want = c_oracle.syndrome_batch(h, r, n, _native.pack_rows(bits), batch)
        for extra in (0, 1, 2):
            e_view, _ = dirty_input(ctx, _native.pack_rows(bits, ld=1 + extra), offsets[0])
            s = out(ctx, batch, 1 + extra, offsets[1])
            ctx.syndrome_dev(chk, e_view, batch, 1 + extra, s.view, 1 + extra)
            s.check(want, preserved=True, what="batch %d pitch %d" % (batch, 1 + extra))


@pytest.mark.parametrize("offsets", OFFSETS, ids=OFFSET_IDS)
@pytest.mark.parametrize("n", [7, 8, 9, 16, 17, 32, 33, 64])
def test_outputs_syndrome_bit_sliced(ctx, n, offsets):
    # even pitches and 16-byte aligned pointers: two words per lane and access; odd pitches or any other address: word by word
    r = max(1, n - 3)
    rng = np.random.default_rng(n)
    hm = rng.integers(0, 2, (r, n))
    h = _native.pack_rows(hm)
    chk = ctx.check_create(h, r, n)
    for words in (1, 2, 3, 301):
        batch = 64 * words - 5                                           # (the last word is a partial one)
        bits = rng.integers(0, 2, (batch, n))
        synd = c_oracle.unpack_rows(c_oracle.syndrome_batch(h, r, n, _native.pack_rows(bits), batch), r)
        want = _native.pack_rows(synd.T)                                 # r rows of `words` words: bit j of word b = sample 64 b + j
        for extra in (0, 1, 2):
            e_view, _ = dirty_input(ctx, _native.pack_rows(bits.T, ld=words + extra), offsets[0])
            s = out(ctx, r, words + extra, offsets[1])
            ctx.syndrome_dev(chk, e_view, batch, words + extra, s.view, words + extra, _native.LAYOUT_BIT_SLICED)
            s.check(want, preserved=True, what="%d words, pitch %d" % (words, words + extra))


def test_outputs_syndrome_tiled_and_sample_major(ctx):
    r, n, batch = 200, 1000, 777
    rng = np.random.default_rng(8)
    h = _native.pack_rows(rng.integers(0, 2, (r, n)))
    e = _native.pack_rows(rng.integers(0, 2, (batch, n)))
    chk = ctx.check_create(h, r, n)
    want = c_oracle.syndrome_batch(h, r, n, e, batch)
    t_view, _ = dirty_input(ctx, _native.tile_rows(e, n))
    for lds in (batch + 1, batch + 2, 832):                              # slab-major: ceil(r / 64) rows of lds > batch words
        s = out(ctx, chk.slabs, lds)
        ctx.syndrome_dev(chk, t_view, batch, 0, s.view, lds, _native.LAYOUT_TILED)
        s.check(np.ascontiguousarray(want.T), preserved=True, what="slab-major, lds %d" % lds)
    for extra in (1, 2):                                                 # sample-major, n > 64: through the workspace
        e_view, _ = dirty_input(ctx, _native.pack_rows(_native.unpack_rows(e, n), ld=e.shape[1] + extra))
        s = out(ctx, batch, chk.slabs + extra)
        ctx.syndrome_dev(chk, e_view, batch, e.shape[1] + extra, s.view, chk.slabs + extra)
        s.check(want, preserved=True, what="sample-major, pitch + %d" % extra)


# ---- outputs and accumulation: gf2_syndrome_sparse_dev ---------------------------------------------------------------------------

#              r, n: all nine EW x SW instantiations of the lane kernel (EW = 2, 4, 8 error words; SW = 1, 2, 4 syndrome words)
LANE_SHAPES = [(10, 65), (64, 129), (64, 257), (65, 128), (128, 256), (128, 512), (129, 128), (192, 256), (256, 512), (129, 257),
               (10, 512)]


def test_lane_shapes_cover_every_instantiation():
    ew = lambda n: 2 if _native.words_for(n) <= 2 else (4 if _native.words_for(n) <= 4 else 8)
    sw = lambda r: 1 if _native.words_for(r) <= 1 else (2 if _native.words_for(r) <= 2 else 4)
    assert {(ew(n), sw(r)) for r, n in LANE_SHAPES} == {(e, s) for e in (2, 4, 8) for s in (1, 2, 4)}
    assert {r for r, _ in LANE_SHAPES} == {10, 64, 65, 128, 129, 192, 256} and {n for _, n in LANE_SHAPES} == {65, 128, 129, 256, 257, 512}


@pytest.mark.parametrize("shape", LANE_SHAPES)
def test_outputs_sparse_lane_kernel(ctx, shape):
    # the kernel stores min(lds, SW) words of a row (rows past r are zero): words past ceil(r / 64) are zeroed or left alone
    r, n = shape
    rng = np.random.default_rng(r * 3 + n)
    h = standard_check(rng, r, n, None)
    chk = ctx.check_create(h, r, n)
    batch = 333
    e = _native.pack_rows((rng.random((batch, n)) < 0.1).astype(np.uint8))
    e[0] = 0
    want = c_oracle.syndrome_batch(h, r, n, e, batch)
    want_h = c_oracle.histogram(want, batch, r, 1, r + 1)
    words = _native.words_for(r)
    sw = 1 if words <= 1 else (2 if words <= 2 else 4)
    for extra in (0, 1, 2):
        e_view, _ = dirty_input(ctx, _native.pack_rows(_native.unpack_rows(e, n), ld=e.shape[1] + extra))
        for lds in sorted({words, words + 1, sw + 1}):
            s = out(ctx, batch, lds)
            hist = out(ctx, 1, r + 1, prefill=ramp(r + 1))
            for _ in range(2):
                ctx.syndrome_sparse_dev(chk, e_view, batch, e.shape[1] + extra, s.view, lds, hist.view, r + 1)
            s.check(want, what="lds %d" % lds)
            hist.check_accumulated(ramp(r + 1), want_h, times=2)


@pytest.mark.parametrize("case", [(65, 200, None, 100), (96, 600, 100, 130), (2047, 4096, 2048, 40)])
def test_outputs_sparse_column_gather(ctx, route, case):
    r, n, ioff, batch = case
    rng = np.random.default_rng(r + n)
    h = standard_check(rng, r, n, ioff)
    chk = ctx.check_create(h, r, n)
    em = (rng.random((batch, n)) < 0.02).astype(np.uint8)
    em[0], em[3] = 0, 1
    e = _native.pack_rows(em)
    want = c_oracle.syndrome_batch(h, r, n, e, batch)
    want_h = c_oracle.histogram(want, batch, r, 1, r + 1)
    route.set_flags(_native.F_SPARSE_GATHER)
    for extra in (0, 1, 2):
        e_view, _ = dirty_input(ctx, _native.pack_rows(em, ld=e.shape[1] + extra))
        lds = want.shape[1] + extra
        s = out(ctx, batch, lds)
        hist = out(ctx, 1, r + 1, prefill=ramp(r + 1))
        ctx.syndrome_sparse_dev(chk, e_view, batch, e.shape[1] + extra, s.view, lds, hist.view, r + 1)
        ctx.syndrome_sparse_dev(chk, e_view, batch, e.shape[1] + extra, None, 0, hist.view, r + 1)       # (the histogram-only kernel)
        s.check(want, what="pitch + %d" % extra)
        hist.check_accumulated(ramp(r + 1), want_h, times=2)
        s2 = out(ctx, batch, lds)
        ctx.syndrome_sparse_dev(chk, e_view, batch, e.shape[1] + extra, s2.view, lds)                    # (the syndromes-only kernel)
        s2.check(want, what="syndromes only, pitch + %d" % extra)


@pytest.mark.parametrize("offsets", OFFSETS, ids=OFFSET_IDS)
def test_outputs_sparse_slabs_and_its_fast_decisions(ctx, route, offsets):
    # the hand-scheduled gather kernel needs 16-byte aligned errors with an even pitch and, to store syndromes, 16-byte aligned
    # syndromes with an even pitch; everything else takes the compiler-scheduled one: identical results
    r, n, ioff, batch = 2047, 4096, 2048, 1500
    rng = np.random.default_rng(r + batch)
    h = standard_check(rng, r, n, ioff)
    chk = ctx.check_create(h, r, n)
    em = (rng.random((batch, n)) < 0.007).astype(np.uint8)
    em[7] = (rng.random(n) < 0.03).astype(np.uint8)                      # beyond a record: finished by the compact kernel
    e = _native.pack_rows(em)
    want = c_oracle.syndrome_batch(h, r, n, e, batch)
    want_h = c_oracle.histogram(want, batch, r, 1, r + 1)
    route.set_flags(_native.F_SPARSE_SLABS)
    for extra in (0, 1, 2):
        e_view, _ = dirty_input(ctx, _native.pack_rows(em, ld=e.shape[1] + extra), offsets[0])
        lds = want.shape[1] + extra
        s = out(ctx, batch, lds, offsets[1])
        hist = out(ctx, 1, r + 1, offsets[1], prefill=ramp(r + 1))
        ctx.syndrome_sparse_dev(chk, e_view, batch, e.shape[1] + extra, s.view, lds, hist.view, r + 1)
        ctx.syndrome_sparse_dev(chk, e_view, batch, e.shape[1] + extra, None, 0, hist.view, r + 1)
        s.check(want, what="pitch + %d" % extra)
        hist.check_accumulated(ramp(r + 1), want_h, times=2)


# ---- accumulation: gf2_histogram_dev ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [_native.LAYOUT_SAMPLE_MAJOR, _native.LAYOUT_TILED], ids=["sample-major", "slab-major"])
@pytest.mark.parametrize("r,mode", [(10, _native.HIST_FULL), (10, _native.HIST_WEIGHT), (14, _native.HIST_FULL), (14, _native.HIST_WEIGHT),
                                    (130, _native.HIST_WEIGHT)])
def test_histogram_accumulates(ctx, r, mode, layout):
    # r = 10: bins privatised in LDS; r = 14, full: 16384 bins, global atomics; r = 130: three words per syndrome
    rng = np.random.default_rng(r + mode)
    nbins = 1 << r if mode == _native.HIST_FULL else r + 1
    words = _native.words_for(r)
    for batch in (1, 2047, 2049):
        s = _native.pack_rows(rng.integers(0, 2, (batch, r)))
        want = c_oracle.histogram(s, batch, r, 0 if mode == _native.HIST_FULL else 1, nbins)
        assert int(want.sum()) == batch
        for extra in (1, 2):
            if layout == _native.LAYOUT_TILED:
                lds = batch + extra
                laid = np.full((words, lds), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)      # (pad words of the input are never read)
                laid[:, :batch] = s.T
            else:
                lds = words + extra
                laid = np.full((batch, lds), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
                laid[:, :words] = s
            s_view, _ = dirty_input(ctx, laid)
            hist = out(ctx, 1, nbins, prefill=ramp(nbins))
            for _ in range(2):
                ctx.histogram_dev(s_view, batch, lds, r, mode, hist.view, nbins, layout)
            hist.check_accumulated(ramp(nbins), want, times=2, what="batch %d" % batch)


@pytest.mark.parametrize("name", ["lane", "column-gather", "slabs"])
def test_sparse_histogram_accumulates(ctx, route, name):
    r, n, ioff, flag = {"lane": (130, 200, None, 0), "column-gather": (100, 300, 100, _native.F_SPARSE_GATHER),
                        "slabs": (100, 300, 100, _native.F_SPARSE_SLABS)}[name]
    rng = np.random.default_rng(r)
    h = standard_check(rng, r, n, ioff)
    chk = ctx.check_create(h, r, n)
    route.set_flags(flag)
    for batch in (1, 2047, 2049):
        e = _native.pack_rows((rng.random((batch, n)) < 0.05).astype(np.uint8))
        want = c_oracle.histogram(c_oracle.syndrome_batch(h, r, n, e, batch), batch, r, 1, r + 1)
        e_view, _ = dirty_input(ctx, e)
        hist = out(ctx, 1, r + 1, prefill=ramp(r + 1))
        for _ in range(2):
            ctx.syndrome_sparse_dev(chk, e_view, batch, e.shape[1], None, 0, hist.view, r + 1)
        hist.check_accumulated(ramp(r + 1), want, times=2, what="batch %d" % batch)


# ---- outputs: the tiled layout and the sampler -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [70, 513, 4096])
def test_outputs_retile_and_sampler(ctx, n):
    count = 65                                                           # two tiles, 63 pad samples in the second
    rng = np.random.default_rng(n)
    words, tiled = _native.words_for(n), _native.tiled_words(n, count)
    bits = rng.integers(0, 2, (count, n))
    want_t = _native.tile_rows(_native.pack_rows(bits), n).reshape(1, tiled)
    for extra in (0, 1, 2):
        e_view, _ = dirty_input(ctx, _native.pack_rows(bits, ld=words + extra))
        t = out(ctx, 1, tiled)
        ctx.retile_dev(e_view, count, words + extra, n, t.view)
        t.check(want_t, what="retile, pitch + %d" % extra)               # the whole buffer is defined: pad samples and the pad word are zero
    want_x, want_z = c_oracle.sample_errors(n, 5, 77, count, 0.05, 0.02, 0.03)
    tx, tz = out(ctx, 1, tiled), out(ctx, 1, tiled)
    ctx.sample_errors_dev(n, 5, 77, count, 0.05, 0.02, 0.03, tx.view, tz.view, 0, _native.LAYOUT_TILED)
    tx.check(_native.tile_rows(want_x, n).reshape(1, tiled), what="tiled e_x")
    tz.check(_native.tile_rows(want_z, n).reshape(1, tiled), what="tiled e_z")
    for extra in (0, 1, 2):
        for lead in (256, 264):                                          # (sample-major rows: any 8-byte-aligned address)
            sx, sz = out(ctx, count, words + extra, lead), out(ctx, count, words + extra, lead)
            ctx.sample_errors_dev(n, 5, 77, count, 0.05, 0.02, 0.03, sx.view, sz.view, words + extra)
            sx.check(want_x, what="e_x, pitch + %d" % extra)
            sz.check(want_z, what="e_z, pitch + %d" % extra)


# ---- outputs: the outcome stores, padding exactly preserved ---------------------------------------------------------------------

def outcomes_of_effects(eff, seed, first, count, p):
    """The outcome words by their definition (include/gf2hip.h): the sampler with n := L draws the faults, an X fault XORs in
    eff[l][0], a Z fault eff[l][1], a Y fault both."""
    locations = eff.shape[0]
    ex, ez = c_oracle.sample_errors(locations, seed, first, count, *p)
    want = np.zeros((count, eff.shape[2]), dtype=np.uint64)
    for c, packed in enumerate((ex, ez)):
        bits = c_oracle.unpack_rows(packed, locations, dtype=bool)
        for i in range(count):
            if bits[i].any():
                want[i] ^= np.bitwise_xor.reduce(eff[bits[i], c, :], axis=0)
    return want


def test_outputs_outcome_stores(ctx):
    code = CSSCode(STEANE, STEANE)
    count, p = 300, (0.02, 0.01, 0.02)
    encoder = circuit_noise.FaultCircuit.for_code(code, circuit_noise.encoder_gates(code, 'zero'))
    program = ft_noise.program_for(code, ("X",))
    cases = [("gf2_circuit_outcomes_dev", ctx.circuit_create(encoder.effects), encoder.effects, ctx.circuit_outcomes_dev),
             ("gf2_ft_outcomes_dev", ctx.ft_circuit_create(program.effects), program.effects, ctx.ft_outcomes_dev)]
    for name, handle, eff, call in cases:
        ldr = eff.shape[2]
        want = outcomes_of_effects(eff, 9, 1000, count, p)
        assert want.any()
        buf = out(ctx, count, ldr + 2)
        call(handle, 9, 1000, count, *p, buf.view, ldr + 2)
        buf.check(want, preserved=True, what=name)
    ref = stream_ref.cycle_reference(code, 2, False)
    gadget = stream_noise.stream_for(code, "cycle", (2, False))
    p = (0.002, 0.001, 0.002)
    want = ref.words(9, 1000, count, p)
    stream = ctx.stream_create(*gadget._sequence())
    buf = out(ctx, count, gadget.ldw + 2)
    ctx.stream_outcomes_dev(stream, 9, 1000, count, *p, buf.view, gadget.ldw + 2)
    buf.check(want, preserved=True, what="gf2_stream_outcomes_dev")


# ---- outputs and alignment: gf2_rref_batch_dev ---------------------------------------------------------------------------------

@pytest.mark.parametrize("lead", [256, 264], ids=["aligned", "matrices+8"])
@pytest.mark.parametrize("shape", [(129, 65, 33), (64, 512, 5), (64, 1024, 5), (128, 200, 3)])
def test_outputs_rref_small_matrices(ctx, shape, lead):
    # rows of whole 16-byte pieces are loaded as such when the batch is 16-byte aligned (64 x 512), four pivots at a time for rows of
    # 16 words (64 x 1024); any other address takes the word-by-word loads of the same kernels
    m, n, batch = shape
    packed, want = rref_reference(m, n, batch)
    rref_dirty(ctx, packed, want, m, n, lead)
    rref_dirty(ctx, packed, want, m, n, lead, with_pivots=False)


def test_outputs_rref_blocked(ctx, route):
    m, n, batch = 300, 600, 4
    packed, want = rref_reference(m, n, batch)
    rref_dirty(ctx, packed, want, m, n)
    rref_dirty(ctx, packed, want, m, n, with_pivots=False)
    # the blocked routes move rows as 16-byte pieces: an address that is not 16-byte aligned is refused on the host, before any launch
    a_view, _ = dirty_input(ctx, packed, 264)
    rank = out(ctx, 1, batch)
    rc = _native.lib().gf2_rref_batch_dev(ctx.handle, a_view.ptr, batch, m, n, packed.shape[2], None, rank.view.ptr)
    assert rc == _native.GF2_E_ARG and b"16-byte aligned" in _native.lib().gf2_last_error()
    rank.check(np.zeros((1, 0), dtype=np.uint64), preserved=True)
    # ... also for a small matrix that GF2_F_RREF_NO_SMALL sends to the blocked route; aligned, that route gives the same result
    small, want_small = rref_reference(64, 512, 5)
    route.set_flags(_native.F_RREF_NO_SMALL)
    rref_dirty(ctx, small, want_small, 64, 512)
    s_view, _ = dirty_input(ctx, small, 264)
    rc = _native.lib().gf2_rref_batch_dev(ctx.handle, s_view.ptr, 5, 64, 512, 8, None, rank.view.ptr)
    assert rc == _native.GF2_E_ARG and b"16-byte aligned" in _native.lib().gf2_last_error()
    rank.check(np.zeros((1, 0), dtype=np.uint64), preserved=True)
