"""
Monte-Carlo syndrome histograms [build-defined, SURVEY.md 8a x3 and 8e].

Every sample is independent and sample i is a pure function of (seed, i), so the global index range
[first, first + count) is cut into contiguous shards, one per GPU / process, with no exchange on the
data path.  The only collective is the final sum of the histograms: one all-reduce of at most
(r_1 + 1) + (r_2 + 1) uint64 bins (about 32 KiB at n = 4096) -- RCCL over xGMI when torch.distributed
runs on the "nccl" backend, gloo on CPU.  The result is identical for every number of shards.
"""
import collections
import fractions as _fractions
import math
import numbers

import numpy as np

from . import _native


def shard_range(first, count, rank, world):
    """Contiguous shard of [first, first + count) for `rank` of `world`: the first (count % world)
    ranks take one extra sample.  Returns (shard_first, shard_count)."""
    if world < 1 or not 0 <= rank < world:
        raise ValueError("bad rank/world")
    base, extra = divmod(int(count), int(world))
    mine = base + (1 if rank < extra else 0)
    start = int(first) + rank * base + min(rank, extra)
    return start, mine


def _rank_world(group=None):
    """(rank, world size) of this process in the torch.distributed group; (0, 1) when no process group is initialised."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def pick_mode(r_1, r_2, mode=None):
    if mode is None:
        mode = 'full' if (r_1 <= 24 and r_2 <= 24) else 'weight'
    if mode not in ('full', 'weight'):
        raise ValueError("mode must be 'full' or 'weight'")
    if mode == 'full' and (r_1 > 24 or r_2 > 24):
        raise ValueError("full histograms need r_1, r_2 <= 24")
    return mode


def run_local(code, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, mode=None):
    """Histograms of samples [first_sample, first_sample + num_samples) on this process's GPU."""
    mode = pick_mode(code.r_1, code.r_2, mode)
    chk1, chk2 = code._device_checks()
    ctx = _native.default_context()
    hist_z, hist_x = ctx.mc_run(chk1, chk2, int(seed), int(first_sample), int(num_samples), float(p_x), float(p_y),
                                float(p_z), _native.HIST_FULL if mode == 'full' else _native.HIST_WEIGHT)
    return {'hist_z': hist_z, 'hist_x': hist_x, 'mode': mode}


def rccl_comm(group=None, ctx=None):
    """A communicator of libgf2hip's own (gf2_comm_create over librccl) spanning the ranks of the torch.distributed group:
    rank 0 makes the id, the group's rendezvous carries its 128 bytes to the others (any backend; gloo needs no GPU
    runtime in torch).  The histogram all-reduce then runs on the compute context's stream from device memory, with no
    second GPU runtime in between.  None when no process group is initialised."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return None
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    box = [None]
    if rank == 0:
        # the id, or the reason there is none (librccl does not load here): every rank must hear of it, or the others would
        # sit in the broadcast for ever
        try:
            box[0] = _native.Comm.unique_id()
        except _native.GF2Error as err:
            box[0] = (err.code, err.message)
    dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    if not isinstance(box[0], bytes):
        raise _native.GF2Error(*box[0])                     # on every rank alike
    return _native.Comm(ctx or _native.default_context(), box[0], world, rank)


def all_reduce_histograms(hists, group=None, device=None, comm=None):
    """Sum a list of uint64 histograms over the ranks (one all-reduce of the concatenation).  With `comm` (a _native.Comm,
    see rccl_comm) the sum runs over libgf2hip's RCCL communicator; otherwise over torch.distributed -- RCCL on the
    "nccl" backend, gloo on CPU; counts stay below 2^63, so the int64 transport is exact.  With neither a communicator nor
    a process group the input is returned unchanged."""
    if comm is not None:
        return comm.allreduce_host(hists)
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return [np.array(h, dtype=np.uint64) for h in hists]
    sizes = [int(h.size) for h in hists]
    flat = np.concatenate([np.asarray(h, dtype=np.uint64).view(np.int64) for h in hists])
    if device is None:
        # RCCL needs the buffer on THIS rank's GPU: the one the compute context runs on (GF2_DEVICE / LOCAL_RANK), not
        # torch's current device, which is cuda:0 in every rank unless the caller set it
        device = torch.device('cuda', _native.default_context().device) if dist.get_backend(group) == 'nccl' else 'cpu'
    buf = torch.from_numpy(flat.copy()).to(device)
    dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
    total = buf.cpu().numpy().view(np.uint64)
    out, pos = [], 0
    for size in sizes:
        out.append(total[pos:pos + size].copy())
        pos += size
    return out


def run_sharded(code, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, mode=None, group=None, local_fn=None, comm=None):
    """This rank's shard of the global range, then the histogram all-reduce (over `comm` when given, see
    all_reduce_histograms).  `local_fn` (same signature as run_local) replaces the GPU computation; the CPU tests of the
    sharding use it."""
    rank, world = _rank_world(group)
    start, mine = shard_range(first_sample, num_samples, rank, world)
    fn = local_fn or run_local
    part = fn(code, mine, p_x, p_y, p_z, seed=seed, first_sample=start, mode=mode)
    hist_z, hist_x = all_reduce_histograms([part['hist_z'], part['hist_x']], group=group, comm=comm)
    return {'hist_z': hist_z, 'hist_x': hist_x, 'mode': part['mode'], 'shard': (start, mine)}


DECODE_FIELDS = ('logical_x', 'logical_z', 'logical_any', 'uncorrectable_x', 'uncorrectable_z')


def dense_table(table, r, n):
    """A syndrome table (dict: vec_to_int(syndrome) -> error vector, css_code.py:715-735) as 2^r packed words
    indexed by the key; entries the table does not have are ~0."""
    out = np.full(1 << r, np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    if len(table):
        keys = np.fromiter((int(key) for key in table), dtype=np.int64, count=len(table))
        errs = np.array(list(table.values()), dtype=np.uint8).reshape(len(table), n)
        out[keys] = _native.pack_rows(errs)[:, 0]                    # (n <= 63: one word per error)
    return out


def packed_word(vec):
    word = 0
    for j in np.flatnonzero(np.asarray(vec)):
        word |= 1 << int(j)
    return word


def table_entries(table, r, n):
    """A syndrome table (dict: vec_to_int(syndrome) -> error vector) as the arrays gf2_mc_decode_hashed takes: keys (entries x 1
    word for r <= 63, x 2 words, low first, beyond) and the packed errors (entries x 2 words, n <= 128)."""
    kw = 1 if r <= 63 else 2
    keys = np.zeros((len(table), kw), dtype=np.uint64)
    mask = (1 << 64) - 1
    if kw == 1:
        keys[:, 0] = np.fromiter((int(key) for key in table), dtype=np.uint64, count=len(table))
    else:
        for i, key in enumerate(table):
            key = int(key)
            keys[i, 0] = key & mask
            keys[i, 1] = key >> 64
    errs = np.array(list(table.values()), dtype=np.uint8).reshape(len(table), n)
    corr = np.zeros((len(table), 2), dtype=np.uint64)
    packed = _native.pack_rows(errs) if len(table) else np.zeros((0, 1), dtype=np.uint64)
    corr[:, :packed.shape[1]] = packed[:, :2]
    return keys, corr


def decode_local(code, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, hashed=None):
    """Table decode + logical-error tally of samples [first_sample, first_sample + num_samples) on this GPU: gf2_mc_decode
    (dense tables of 2^r words) for n <= 63 and r_1, r_2 <= 20, gf2_mc_decode_hashed (the tables' entries in hash tables on the
    device) for every other code of at most 128 qubits.  Returns a dict of counts (DECODE_FIELDS) plus 'samples'."""
    if code.n > 128 or max(code.r_1, code.r_2) > 127 or min(code.r_1, code.r_2) < 1:
        raise ValueError("table decode needs n <= 128 and 1 <= r_1, r_2 <= 127")
    ctx = _native.default_context()
    if hashed or code.n > 63 or code.r_1 > 20 or code.r_2 > 20:      # (hashed=True: the hash-table kernel for a small code too)
        two = lambda vec: np.pad(_native.pack_rows(np.asarray(vec).reshape(1, -1))[0], (0, 2))[:2]
        # (the tables as arrays: made once per code object -- 0.1 s of Python for a table of 350 000 entries)
        cached = getattr(code, "_hashed_table_arrays", None)
        if cached is None or cached[0] is not code._c1_syndromes or cached[1] is not code._c2_syndromes:
            cached = (code._c1_syndromes, code._c2_syndromes, table_entries(code._c1_syndromes, code.r_1, code.n),
                      table_entries(code._c2_syndromes, code.r_2, code.n))
            code._hashed_table_arrays = cached
        (keys1, corr1), (keys2, corr2) = cached[2], cached[3]
        counts = ctx.mc_decode_hashed(code.n, _native.pack_rows(code.parity_check_c1), code.r_1, keys1, corr1,
                                      _native.pack_rows(code.parity_check_c2), code.r_2, keys2, corr2,
                                      two(code.x_operator_matrix()[0]), two(code.z_operator_matrix()[0]),
                                      int(seed), int(first_sample), int(num_samples), float(p_x), float(p_y), float(p_z))
        out = {name: int(v) for name, v in zip(DECODE_FIELDS, counts)}
        out['samples'] = int(num_samples)
        return out
    chk1, chk2 = code._device_checks()
    cached = getattr(code, "_dense_table_arrays", None)             # (made once per code object, like the hash tables' arrays)
    if cached is None or cached[0] is not code._c1_syndromes or cached[1] is not code._c2_syndromes:
        cached = (code._c1_syndromes, code._c2_syndromes, dense_table(code._c1_syndromes, code.r_1, code.n),
                  dense_table(code._c2_syndromes, code.r_2, code.n))
        code._dense_table_arrays = cached
    counts = ctx.mc_decode(chk1, chk2, cached[2], cached[3],
                           packed_word(code.x_operator_matrix()[0]), packed_word(code.z_operator_matrix()[0]),
                           int(seed), int(first_sample), int(num_samples), float(p_x), float(p_y), float(p_z))
    out = {name: int(v) for name, v in zip(DECODE_FIELDS, counts)}
    out['samples'] = int(num_samples)
    return out


def decode_sharded(code, num_samples, p_x, p_y, p_z, seed=0, first_sample=0, group=None, local_fn=None):
    """This rank's shard of the global range, then one all-reduce of the five counts."""
    rank, world = _rank_world(group)
    start, mine = shard_range(first_sample, num_samples, rank, world)
    part = (local_fn or decode_local)(code, mine, p_x, p_y, p_z, seed=seed, first_sample=start)
    total, = all_reduce_histograms([np.array([part[f] for f in DECODE_FIELDS], dtype=np.uint64)], group=group)
    out = {name: int(v) for name, v in zip(DECODE_FIELDS, total)}
    out['samples'] = int(num_samples)
    return out


# ---- weight-stratified Monte-Carlo (DESIGN.md "Strata") -------------------------------------------------------------------

def binomial_weights(nb, p_t):
    """B_w = C(nb, w) p_t^w (1 - p_t)^(nb - w) for w = 0 .. nb as float64, in log space (log C(nb, w) as a running sum of
    log((nb - i) / (i + 1)), log1p for the complement), so that B_w keeps its relative accuracy at p_t = 1e-12 and below."""
    nb, p_t = int(nb), float(p_t)
    if nb < 0 or not 0.0 <= p_t <= 1.0:
        raise ValueError("binomial weights need nb >= 0 and 0 <= p_t <= 1")
    out = np.zeros(nb + 1)
    if p_t == 0.0 or p_t == 1.0:
        out[0 if p_t == 0.0 else nb] = 1.0
        return out
    w = np.arange(nb + 1, dtype=np.float64)
    log_c = np.concatenate(([0.0], np.cumsum(np.log((nb - w[:-1]) / (w[:-1] + 1.0)))))
    return np.exp(log_c + w * np.log(p_t) + (nb - w) * np.log1p(-p_t))


# Strata.rate's result: the logical error rate lies in [estimate, estimate + truncation] up to the statistical error `stderr`.
StratifiedRate = collections.namedtuple('StratifiedRate', ('estimate', 'stderr', 'truncation'))


class Strata(object):
    """Tallies of a stratified run over `nb` positions (the qubits of a code, the fault locations of a circuit): `weights`
    (nstrata, distinct), `samples` (N_w per stratum) and `counts` (nstrata x 5 in DECODE_FIELDS order).  One set of strata serves
    every physical rate: rate(p_t) combines them with binomial weights computed in double precision on the host, so nothing
    is lost below 2^-32."""

    def __init__(self, nb, weights, samples, counts, kinds=(1, 1, 1)):
        self.nb = int(nb)
        self.weights = np.asarray(weights, dtype=np.int64).reshape(-1).copy()
        self.samples = np.asarray(samples, dtype=np.int64).reshape(-1).copy()
        self.counts = np.asarray(counts, dtype=np.uint64).reshape(len(self.weights), len(DECODE_FIELDS)).copy()
        self.kinds = tuple(float(k) for k in kinds)
        if self.samples.shape != self.weights.shape:
            raise ValueError("one sample count per stratum")
        if len(set(self.weights.tolist())) != len(self.weights):
            raise ValueError("the weights of the strata must be distinct")
        if len(self.weights) and (self.weights.min() < 0 or self.weights.max() > self.nb):
            raise ValueError("a stratum's weight lies in [0, nb]")

    def fractions(self, field='logical_any'):
        """f_w estimates: counts / samples per stratum (0 where a stratum has no samples)."""
        col = self.counts[:, DECODE_FIELDS.index(field)].astype(np.float64)
        return np.divide(col, self.samples, out=np.zeros(len(col)), where=self.samples > 0)

    def rate(self, p_t, field='logical_any'):
        """The rate of `field` at total physical error probability p_t per position (kinds in the ratio the strata were drawn
        with): estimate sum_w B_w f_w, its standard error sqrt(sum_w B_w^2 f_w (1 - f_w) / N_w), and `truncation`, the binomial
        mass of the weights without samples -- a rigorous additive upper bound, since every f_w <= 1."""
        b_all = binomial_weights(self.nb, p_t)
        live = self.samples > 0
        b = b_all[self.weights[live]]
        f = self.fractions(field)[live]
        sampled = np.zeros(self.nb + 1, dtype=bool)
        sampled[self.weights[live]] = True
        return StratifiedRate(math.fsum(b * f), math.sqrt(math.fsum(b * b * f * (1.0 - f) / self.samples[live])),
                              math.fsum(b_all[~sampled]))

    def curve(self, p_values, field='logical_any'):
        """rate() at every p of p_values: (estimates, stderrs, truncations) as arrays."""
        rows = np.array([self.rate(p, field) for p in p_values], dtype=np.float64).reshape(-1, 3)
        return rows[:, 0], rows[:, 1], rows[:, 2]

    def as_dicts(self):
        return [dict(zip(DECODE_FIELDS, (int(v) for v in row)), weight=int(w), samples=int(n))
                for w, n, row in zip(self.weights, self.samples, self.counts)]


def _strata_request(weights, samples, kinds, first_sample):
    weights = [int(w) for w in np.asarray(weights).reshape(-1)]
    samples = np.broadcast_to(np.asarray(samples, dtype=np.int64), (len(weights),)).copy()
    firsts = np.broadcast_to(np.asarray(first_sample, dtype=np.int64), (len(weights),)).copy()
    kinds = tuple(float(k) for k in kinds)
    if len(kinds) != 3 or min(kinds) < 0 or not sum(kinds) > 0:
        raise ValueError("kinds are three non-negative weights (X, Y, Z) with a positive sum")
    if samples.size and samples.min() < 0:
        raise ValueError("negative sample count")
    return weights, samples, firsts, kinds


def _strata_calls(firsts):
    """Strata grouped by their first sample: one native call (one set of hash tables) per distinct value."""
    groups = {}
    for s, first in enumerate(firsts.tolist()):
        groups.setdefault(first, []).append(s)
    return groups.items()


def strata_local(code, weights, samples, kinds=(1, 1, 1), seed=0, first_sample=0):
    """Stratified table decode on this GPU (gf2_mc_decode_strata): stratum s draws samples [first_sample, first_sample + samples[s])
    of exactly weights[s] errors on the code's n qubits, kinds X : Y : Z = kinds.  `samples` and `first_sample` are one number for
    all strata or one per stratum.  Returns a Strata."""
    if code.n > 128 or max(code.r_1, code.r_2) > 127 or min(code.r_1, code.r_2) < 1:
        raise ValueError("table decode needs n <= 128 and 1 <= r_1, r_2 <= 127")
    weights, samples, firsts, kinds = _strata_request(weights, samples, kinds, first_sample)
    if any(w < 0 or w > code.n for w in weights):
        raise ValueError("a stratum's weight lies in [0, n = %d]" % code.n)
    two = lambda vec: np.pad(_native.pack_rows(np.asarray(vec).reshape(1, -1))[0], (0, 2))[:2]
    cached = getattr(code, "_hashed_table_arrays", None)             # (shared with decode_local)
    if cached is None or cached[0] is not code._c1_syndromes or cached[1] is not code._c2_syndromes:
        cached = (code._c1_syndromes, code._c2_syndromes, table_entries(code._c1_syndromes, code.r_1, code.n),
                  table_entries(code._c2_syndromes, code.r_2, code.n))
        code._hashed_table_arrays = cached
    (keys1, corr1), (keys2, corr2) = cached[2], cached[3]
    ctx = _native.default_context()
    counts = np.zeros((len(weights), len(DECODE_FIELDS)), dtype=np.uint64)
    for first, rows in _strata_calls(firsts):
        counts[rows] = ctx.mc_decode_strata(code.n, _native.pack_rows(code.parity_check_c1), code.r_1, keys1, corr1,
                                            _native.pack_rows(code.parity_check_c2), code.r_2, keys2, corr2,
                                            two(code.x_operator_matrix()[0]), two(code.z_operator_matrix()[0]), int(seed), int(first),
                                            [weights[s] for s in rows], samples[rows], *kinds)
    return Strata(code.n, weights, samples, counts, kinds)


def strata_sharded(code, weights, samples, kinds=(1, 1, 1), seed=0, first_sample=0, group=None, local_fn=None):
    """Every stratum's sample range cut into this rank's shard (shard_range), then one all-reduce of the nstrata x 5 counts.
    `local_fn` (strata_local's signature; FaultCircuit.strata_local for a circuit) replaces the computation."""
    rank, world = _rank_world(group)
    weights, samples, firsts, kinds = _strata_request(weights, samples, kinds, first_sample)
    shards = [shard_range(first, count, rank, world) for first, count in zip(firsts.tolist(), samples.tolist())]
    part = (local_fn or strata_local)(code, weights, [mine for _, mine in shards], kinds=kinds, seed=seed,
                                      first_sample=[start for start, _ in shards])
    total, = all_reduce_histograms([part.counts.reshape(-1)], group=group)
    return Strata(part.nb, weights, samples, total, kinds)


# ---- exact strata (DESIGN.md "Exact strata") --------------------------------------------------------------------------------

def _kind_ratio(kinds):
    kinds = tuple(kinds)
    if len(kinds) != 3 or min(kinds) < 0 or not sum(kinds) > 0:
        raise ValueError("kinds are three non-negative weights (X, Y, Z) with a positive sum")
    return kinds


def _same_ratio(a, b):
    """Kind weights that differ by a positive factor only."""
    sa, sb = sum(a), sum(b)
    return all(abs(float(x) * float(sb) - float(y) * float(sa)) <= 1e-12 * float(sa) * float(sb) for x, y in zip(a, b))


class ExactStrata(object):
    """Whole strata counted, not sampled: `weights` (distinct) over `nb` positions and, per weight w, the (w + 1, w + 1, 5) uint64
    counts [n_x][n_y][field] of FaultCircuit.enumerate_strata over ALL C(nb, w) subsets (the sum of the parts of a sharded or
    windowed enumeration).  The counts are kept per kind composition, so one enumeration serves every physical rate and every
    X : Y : Z ratio:  f_w = sum counts[n_x][n_y] k_x^n_x k_y^n_y k_z^n_z / (s^w C(nb, w)),  s = k_x + k_y + k_z."""

    def __init__(self, nb, weights, counts):
        self.nb = int(nb)
        self.weights = [int(w) for w in np.asarray(weights).reshape(-1)]
        if len(set(self.weights)) != len(self.weights):
            raise ValueError("the weights of the strata must be distinct")
        if any(w < 0 or w > self.nb for w in self.weights):
            raise ValueError("a stratum's weight lies in [0, nb]")
        counts = list(counts)
        if len(counts) != len(self.weights):
            raise ValueError("one array of counts per weight")
        self.counts = [np.asarray(c, dtype=np.uint64).reshape(w + 1, w + 1, len(DECODE_FIELDS)).copy() for w, c in zip(self.weights, counts)]

    def configurations(self):
        """3^w C(nb, w) per weight."""
        return [3**w * math.comb(self.nb, w) for w in self.weights]

    def fractions(self, kinds=(1, 1, 1), field='logical_any'):
        """f_w per enumerated weight for kinds X : Y : Z = kinds: exact fractions.Fraction when the three are integers or Fractions,
        floats otherwise."""
        kinds = _kind_ratio(kinds)
        exact = all(isinstance(k, numbers.Rational) for k in kinds)
        k_x, k_y, k_z = (_fractions.Fraction(k) for k in kinds) if exact else (float(k) for k in kinds)
        col, s, out = DECODE_FIELDS.index(field), k_x + k_y + k_z, []
        for w, counts in zip(self.weights, self.counts):
            total = 0
            for n_x in range(w + 1):
                for n_y in range(w + 1 - n_x):
                    c = int(counts[n_x, n_y, col])
                    if c:
                        total += c * k_x**n_x * k_y**n_y * k_z**(w - n_x - n_y)
            out.append(total / (s**w * math.comb(self.nb, w)))
        return out

    def rate(self, p_t, kinds=(1, 1, 1), field='logical_any'):
        """sum_w B_w f_w over the enumerated weights: no statistical error, and `truncation` is the binomial mass of the others."""
        b_all = binomial_weights(self.nb, p_t)
        have = np.zeros(self.nb + 1, dtype=bool)
        have[self.weights] = True
        f = [float(v) for v in self.fractions(kinds, field)]
        return StratifiedRate(math.fsum(b_all[w] * v for w, v in zip(self.weights, f)), 0.0, math.fsum(b_all[~have]))

    def leading_order(self, kinds=(1, 1, 1), field='logical_any'):
        """(w*, c): the smallest enumerated weight with f_w* > 0 and the coefficient c = C(nb, w*) f_w* of p^w* in the rate; None
        when every enumerated stratum is clean."""
        f = dict(zip(self.weights, self.fractions(kinds, field)))
        for w in sorted(f):
            if f[w] > 0:
                return w, math.comb(self.nb, w) * f[w]
        return None

    def merged(self, strata, kinds=None):
        """These strata with the sampled ones of `strata` (a Strata or several): see MergedStrata."""
        return MergedStrata(self, [strata] if isinstance(strata, Strata) else list(strata), kinds)


class MergedStrata(object):
    """Strata's interface over exact and sampled strata together: the exact f_w where there is one (no variance, and the weight
    counts as covered for `truncation`), the sampled estimate elsewhere.  The sampled strata must cover the same nb positions and
    all be drawn with one kind ratio (that of `kinds`, when given), which is then the ratio of the exact fractions too."""

    def __init__(self, exact, sampled, kinds=None):
        self.exact, self.sampled, self.nb = exact, list(sampled), exact.nb
        if kinds is None:
            if not self.sampled:
                raise ValueError("kinds are needed when there are no sampled strata")
            kinds = self.sampled[0].kinds
        self.kinds = _kind_ratio(kinds)
        seen = set()
        for part in self.sampled:
            if part.nb != self.nb:
                raise ValueError("sampled strata over %d positions, exact ones over %d" % (part.nb, self.nb))
            if not _same_ratio(part.kinds, self.kinds):
                raise ValueError("sampled strata drawn with kinds %r do not match %r" % (part.kinds, self.kinds))
            live = set(part.weights[part.samples > 0].tolist())
            if live & seen:
                raise ValueError("two sampled strata of one weight")
            seen |= live
        self.weights = np.array(sorted(set(exact.weights) | seen), dtype=np.int64)

    def _parts(self, field):
        """weight -> (f_w, N_w), N_w = 0 for an exact stratum."""
        out = {}
        for part in self.sampled:
            for w, n, f in zip(part.weights.tolist(), part.samples.tolist(), part.fractions(field)):
                if n > 0:
                    out[w] = (float(f), n)
        for w, f in zip(self.exact.weights, self.exact.fractions(self.kinds, field)):
            out[w] = (float(f), 0)
        return out

    def fractions(self, field='logical_any'):
        parts = self._parts(field)
        return np.array([parts[w][0] for w in self.weights.tolist()])

    def rate(self, p_t, field='logical_any'):
        b_all = binomial_weights(self.nb, p_t)
        parts = self._parts(field)
        have = np.zeros(self.nb + 1, dtype=bool)
        have[self.weights] = True
        return StratifiedRate(math.fsum(b_all[w] * f for w, (f, n) in parts.items()),
                              math.sqrt(math.fsum(b_all[w]**2 * f * (1.0 - f) / n for w, (f, n) in parts.items() if n > 0)),
                              math.fsum(b_all[~have]))

    def curve(self, p_values, field='logical_any'):
        rows = np.array([self.rate(p, field) for p in p_values], dtype=np.float64).reshape(-1, 3)
        return rows[:, 0], rows[:, 1], rows[:, 2]


class PostSelectedStrata(object):
    """Exact strata of a post-selected gadget (ec_noise.ECCircuit / ft_noise.FTProgram.enumerate_strata): `weights` (distinct) over
    `nb` positions and, per weight w, the (w + 1, w + 1, F) uint64 counts [n_x][n_y][field] over ALL C(nb, w) subsets, `fields`
    naming the F columns.  Field 0 is 'accepted'; every other field counts among accepted configurations.  With kind weights
    (k_x, k_y, k_z) of sum s,  A_w(field) = sum counts[n_x][n_y][field] k_x^n_x k_y^n_y k_z^n_z / s^w,  and at total fault
    probability p per position  P(accepted and field) = sum_w A_w p^w (1 - p)^(nb - w).  The fields whose value per configuration
    is 0 or 1 are indicators; the others (`SUM_FIELDS`) are sums, for which a rate has no bounds but a series is the series of the
    conditional expectation."""

    SUM_FIELDS = ('trial_wrong', 'unmatched_x', 'unmatched_z', 'round_unmatched_x', 'round_unmatched_z')

    def __init__(self, nb, weights, counts, fields):
        self.nb = int(nb)
        self.fields = tuple(fields)
        if not self.fields or self.fields[0] != 'accepted':
            raise ValueError("the first field of a post-selected tally is 'accepted'")
        self.weights = [int(w) for w in np.asarray(weights).reshape(-1)]
        if len(set(self.weights)) != len(self.weights):
            raise ValueError("the weights of the strata must be distinct")
        if any(w < 0 or w > self.nb for w in self.weights):
            raise ValueError("a stratum's weight lies in [0, nb]")
        counts = list(counts)
        if len(counts) != len(self.weights):
            raise ValueError("one array of counts per weight")
        self.counts = [np.asarray(c, dtype=np.uint64).reshape(w + 1, w + 1, len(self.fields)).copy() for w, c in zip(self.weights, counts)]

    def configurations(self):
        """3^w C(nb, w) per weight."""
        return [3**w * math.comb(self.nb, w) for w in self.weights]

    def _column(self, field):
        if field not in self.fields:
            raise ValueError("no field %r (the fields are %s)" % (field, ', '.join(self.fields)))
        return self.fields.index(field)

    def coefficients(self, kinds=(1, 1, 1), field='accepted'):
        """A_w(field) per enumerated weight: exact fractions.Fraction when the kinds are integers or Fractions, floats otherwise."""
        kinds = _kind_ratio(kinds)
        exact = all(isinstance(k, numbers.Rational) for k in kinds)
        k_x, k_y, k_z = (_fractions.Fraction(k) for k in kinds) if exact else (float(k) for k in kinds)
        col, s, out = self._column(field), k_x + k_y + k_z, []
        for w, counts in zip(self.weights, self.counts):
            total = _fractions.Fraction(0) if exact else 0.0
            for n_x in range(w + 1):
                for n_y in range(w + 1 - n_x):
                    c = int(counts[n_x, n_y, col])
                    if c:
                        total += c * k_x**n_x * k_y**n_y * k_z**(w - n_x - n_y)
            out.append(total / s**w)
        return out

    def joint(self, p_t, kinds=(1, 1, 1), field='accepted'):
        """P(accepted and field) at total fault probability p_t per position, over the enumerated weights: sum_w A_w p^w
        (1 - p)^(nb - w) = sum_w (A_w / C(nb, w)) B_w with binomial_weights' B_w (log space: accurate at p_t = 1e-12 and below).
        For a sum field, the expectation of the field over accepted configurations times P(accepted)."""
        b_all = binomial_weights(self.nb, p_t)
        return math.fsum(float(a_w / math.comb(self.nb, w)) * b_all[w] for w, a_w in zip(self.weights, self.coefficients(kinds, field)))

    def _missing_mass(self, p_t):
        b_all = binomial_weights(self.nb, p_t)
        have = np.zeros(self.nb + 1, dtype=bool)
        have[self.weights] = True
        return math.fsum(b_all[~have])

    def rate(self, p_t, kinds=(1, 1, 1), field='wrong'):
        """The conditional rate P(field | accepted) of an indicator field as (estimate, lower, upper): with N = joint(field),
        D = joint('accepted') and T the binomial mass of the weights not enumerated, estimate = N / D, lower = N / (D + T), upper =
        (N + T) / (D + T).  The bounds are rigorous: the missing weights add n to N and d to D with 0 <= n <= d <= T."""
        if field in self.SUM_FIELDS:
            raise ValueError("rate() is defined for indicator fields; %r is a sum (series() gives its conditional expectation)" % (field,))
        n, d, t = self.joint(p_t, kinds, field), self.joint(p_t, kinds, 'accepted'), self._missing_mass(p_t)
        if not d > 0:
            raise ValueError("no accepted configuration among the enumerated weights at p_t = %r" % (p_t,))
        return n / d, n / (d + t), (n + t) / (d + t)

    def acceptance(self, p_t, kinds=(1, 1, 1)):
        """(D, D + T): bounds on the probability that an attempt is accepted; their reciprocals bound the expected number of
        attempts of repeat-until-success."""
        d = self.joint(p_t, kinds, 'accepted')
        return d, d + self._missing_mass(p_t)

    def series(self, kinds=(1, 1, 1), field='wrong', order=None):
        """The Taylor coefficients [c_0, ..., c_m] in p_t of the conditional rate of `field` (for a sum field: of its conditional
        expectation), exact for rational kinds.  m (or `order`, if smaller) is the largest order with every weight 0 .. m
        enumerated.  (1 - p)^nb cancels in N / D, which leaves the quotient of sum A_w(field) x^w by sum A_w(accepted) x^w in
        x = p / (1 - p) = p + p^2 + ..., re-expanded in p.  Needs A_0(accepted) = 1 (no fault: accepted), ValueError otherwise."""
        have = set(self.weights)
        m = -1
        while m + 1 in have:
            m += 1
        if m < 0:
            raise ValueError("a series needs the stratum of weight 0")
        if order is not None:
            if int(order) < 0 or int(order) > m:
                raise ValueError("order %d outside [0, %d], the weights enumerated without a gap" % (int(order), m))
            m = int(order)
        at = {w: i for i, w in enumerate(self.weights)}
        num_all, den_all = self.coefficients(kinds, field), self.coefficients(kinds, 'accepted')
        num = [num_all[at[w]] for w in range(m + 1)]
        den = [den_all[at[w]] for w in range(m + 1)]
        if den[0] != 1:
            raise ValueError("a series needs A_0(accepted) = 1, got %r" % (den[0],))
        q = []                                                       # num / den as a power series in x
        for k in range(m + 1):
            q.append(num[k] - sum(q[i] * den[k - i] for i in range(k)))
        # x^j = p^j (1 - p)^-j = sum_k C(k - 1, j - 1) p^k for j >= 1
        out = [q[0]] + [sum(q[j] * math.comb(k - 1, j - 1) for j in range(1, k + 1)) for k in range(1, m + 1)]
        return out

    def leading_order(self, kinds=(1, 1, 1), field='wrong'):
        """(m, c_m): the first non-zero coefficient of series(); None when every coefficient is zero."""
        for k, c in enumerate(self.series(kinds, field)):
            if c != 0:
                return k, c
        return None

    def merged(self, sampled, kinds=None):
        """These strata with the sampled ones of `sampled` (a SampledPostSelectedStrata or several): see MergedPostSelectedStrata."""
        return MergedPostSelectedStrata(self, [sampled] if isinstance(sampled, SampledPostSelectedStrata) else list(sampled), kinds)


# ---- exact strata under gate-level faults ---------------------------------------------------------------

def _series_mul(f, g, m):
    """The product of two power series given by their coefficients, truncated after order m."""
    out = [_fractions.Fraction(0)] * (m + 1)
    for i, a in enumerate(f[:m + 1]):
        if a:
            for j, b in enumerate(g[:m + 1 - i]):
                out[i + j] += a * b
    return out


class GateStrata(object):
    """Exact strata of a post-selected gadget under gate-level faults (ec_noise.ECCircuit / ft_noise.FTProgram.enumerate_gate_strata):
    `n1` one-operand gates and `n2` CNOTs, `weights` (distinct, <= 4) and, per weight w, the (w + 1, w + 1, F) uint64 counts
    [b][c][field] over ALL configurations of w faulty gates of which b are CNOTs, c of those with a two-operand kind; `fields` names
    the F columns, field 0 is 'accepted'.  A model gives the odds (x, y1, y2) of one specific kind against "no fault at this site" --
    x on a one-operand gate, y1 for a one-operand CNOT kind, y2 for a two-operand one -- and
    P(accepted and field) = Z sum counts[w][b][c] x^(w - b) y1^(b - c) y2^c,  Z = (1 + 3 x)^-n1 (1 + 6 y1 + 9 y2)^-n2."""

    SUM_FIELDS = PostSelectedStrata.SUM_FIELDS

    def __init__(self, n1, n2, weights, counts, fields):
        self.n1, self.n2 = int(n1), int(n2)
        self.fields = tuple(fields)
        if not self.fields or self.fields[0] != 'accepted':
            raise ValueError("the first field of a post-selected tally is 'accepted'")
        self.weights = [int(w) for w in np.asarray(weights).reshape(-1)]
        if len(set(self.weights)) != len(self.weights):
            raise ValueError("the weights of the strata must be distinct")
        if any(w < 0 or w > self.n1 + self.n2 for w in self.weights):
            raise ValueError("a stratum's weight lies in [0, n1 + n2]")
        counts = list(counts)
        if len(counts) != len(self.weights):
            raise ValueError("one array of counts per weight")
        self.counts = [np.asarray(c, dtype=np.uint64).reshape(w + 1, w + 1, len(self.fields)).copy() for w, c in zip(self.weights, counts)]

    def configurations(self):
        """sum_b C(n1, w - b) C(n2, b) 3^(w - b) 15^b per weight."""
        return [sum(math.comb(self.n1, w - b) * math.comb(self.n2, b) * 3**(w - b) * 15**b for b in range(w + 1)) for w in self.weights]

    def _column(self, field):
        if field not in self.fields:
            raise ValueError("no field %r (the fields are %s)" % (field, ', '.join(self.fields)))
        return self.fields.index(field)

    @staticmethod
    def depolarising_odds(p1, p2):
        """Depolarising gate faults: a one-operand gate fails with probability p1 (X, Y, Z alike), a CNOT with p2 (its 15 Paulis alike)."""
        p1, p2 = float(p1), float(p2)
        if not (0.0 <= p1 < 1.0 and 0.0 <= p2 < 1.0):
            raise ValueError("the odds need 0 <= p < 1")
        y = p2 / (15.0 * (1.0 - p2))
        return p1 / (3.0 * (1.0 - p1)), y, y

    @staticmethod
    def independent_odds(p):
        """The independent-operand model of the location strata at total probability p per location: a CNOT's two operands fail
        independently, so a two-operand kind has the odds of two faults."""
        p = float(p)
        if not 0.0 <= p < 1.0:
            raise ValueError("the odds need 0 <= p < 1")
        x = p / (3.0 * (1.0 - p))
        return x, x, x * x

    def _terms(self, col):
        for w, counts in zip(self.weights, self.counts):
            for b in range(w + 1):
                for c in range(b + 1):
                    n = int(counts[b, c, col])
                    if n:
                        yield n, w - b, b - c, c

    def joint(self, odds, field='accepted'):
        """P(accepted and field) over the enumerated weights at the odds (x, y1, y2), every term in log space like binomial_weights:
        accurate at p = 1e-12 and below.  For a sum field, the expectation of the field over accepted configurations times
        P(accepted)."""
        x, y1, y2 = (float(v) for v in odds)
        if min(x, y1, y2) < 0.0:
            raise ValueError("odds are not negative")
        log_z = -self.n1 * math.log1p(3.0 * x) - self.n2 * math.log1p(6.0 * y1 + 9.0 * y2)
        terms = []
        for n, e_x, e_1, e_2 in self._terms(self._column(field)):
            if any(e and not v for e, v in ((e_x, x), (e_1, y1), (e_2, y2))):
                continue
            log_t = sum(e * math.log(v) for e, v in ((e_x, x), (e_1, y1), (e_2, y2)) if e)
            terms.append(n * math.exp(log_t + log_z))
        return math.fsum(terms)

    def _missing_mass(self, odds):
        """T: the probability that the number of faulty gates is not an enumerated weight (the sum of two binomials)."""
        x, y1, y2 = (float(v) for v in odds)
        q_1, q_2 = 3.0 * x / (1.0 + 3.0 * x), (6.0 * y1 + 9.0 * y2) / (1.0 + 6.0 * y1 + 9.0 * y2)
        total = np.convolve(binomial_weights(self.n1, q_1), binomial_weights(self.n2, q_2))
        have = np.zeros(len(total), dtype=bool)
        have[self.weights] = True
        return math.fsum(total[~have])

    def acceptance(self, odds):
        """(D, D + T): bounds on the probability that an attempt is accepted."""
        d = self.joint(odds, 'accepted')
        return d, d + self._missing_mass(odds)

    def rate(self, odds, field='wrong'):
        """The conditional rate P(field | accepted) of an indicator field as (estimate, lower, upper), PostSelectedStrata.rate's
        argument: with N = joint(field), D = joint('accepted') and T the probability that the number of faulty gates is not an
        enumerated weight, estimate = N / D, lower = N / (D + T), upper = (N + T) / (D + T)."""
        if field in self.SUM_FIELDS:
            raise ValueError("rate() is defined for indicator fields; %r is a sum (series() gives its conditional expectation)" % (field,))
        n, d, t = self.joint(odds, field), self.joint(odds, 'accepted'), self._missing_mass(odds)
        if not d > 0:
            raise ValueError("no accepted configuration among the enumerated weights at the odds %r" % (tuple(odds),))
        return n / d, n / (d + t), (n + t) / (d + t)

    def _odds_series(self, model, m):
        """(x, y1, y2) as power series in p truncated after order m, exact."""
        one = _fractions.Fraction(1)
        geometric = lambda r, scale: [_fractions.Fraction(0)] + [r**k / scale for k in range(1, m + 1)]   # r p / (scale (1 - r p))
        if model == 'independent':
            x = geometric(one, 3)
            return x, x, _series_mul(x, x, m)
        if isinstance(model, (tuple, list)) and len(model) == 2 and model[0] == 'depolarising' and isinstance(model[1], numbers.Rational):
            if model[1] < 0:
                raise ValueError("the ratio p_2 / p_1 is not negative")
            y = geometric(_fractions.Fraction(model[1]), 15)
            return geometric(one, 3), y, y
        raise ValueError("a model is 'independent' or ('depolarising', r) with r = p_2 / p_1 rational, got %r" % (model,))

    def series(self, model, field='wrong', order=None):
        """The Taylor coefficients [c_0, ..., c_m] in p of the conditional rate of `field` (for a sum field: of its conditional
        expectation), exact fractions.Fraction.  model: ('depolarising', r) with p_1 = p, p_2 = r p, r rational, or 'independent'
        (p per location).  m (or `order`, if smaller) is the largest order with every weight 0 .. m enumerated: a configuration
        of w faulty gates enters at order w or above.  Z cancels in N / D, which leaves a quotient of polynomials in the odds,
        themselves truncated power series in p.  Needs counts[0]['accepted'] = 1 (no fault: accepted), ValueError otherwise."""
        have = set(self.weights)
        m = -1
        while m + 1 in have:
            m += 1
        if m < 0:
            raise ValueError("a series needs the stratum of weight 0")
        if order is not None:
            if int(order) < 0 or int(order) > m:
                raise ValueError("order %d outside [0, %d], the weights enumerated without a gap" % (int(order), m))
            m = int(order)
        odds = self._odds_series(model, m)
        unit = [_fractions.Fraction(1)] + [_fractions.Fraction(0)] * m
        powers = [[unit], [unit], [unit]]
        for v, table in zip(odds, powers):
            for _ in range(m):
                table.append(_series_mul(table[-1], v, m))

        def poly(col):
            total = [_fractions.Fraction(0)] * (m + 1)
            for n, e_x, e_1, e_2 in self._terms(col):
                if e_x + e_1 + e_2 > m:
                    continue
                term = _series_mul(_series_mul(powers[0][e_x], powers[1][e_1], m), powers[2][e_2], m)
                total = [t + n * v for t, v in zip(total, term)]
            return total

        num, den = poly(self._column(field)), poly(0)
        if den[0] != 1:
            raise ValueError("a series needs one accepted configuration of weight 0, got %r" % (den[0],))
        out = []
        for k in range(m + 1):
            out.append(num[k] - sum(out[i] * den[k - i] for i in range(k)))
        return out

    def leading_order(self, model, field='wrong'):
        """(m, c_m): the first non-zero coefficient of series(); None when every coefficient is zero."""
        for k, c in enumerate(self.series(model, field)):
            if c != 0:
                return k, c
        return None

    def merged(self, sampled):
        """These exact strata with sampled ones (a SampledGateStrata or a list of them) as a MergedGateStrata."""
        return MergedGateStrata(self, [sampled] if isinstance(sampled, SampledGateStrata) else list(sampled))


# ---- malignant fault sets of a post-selected gadget (DESIGN.md "Malignant fault sets of the cycle", "... of the measurement") --------

class FaultList(object):
    """The listed fault configurations of a post-selected gadget (ec_noise.ECCircuit / ft_noise.FTProgram.malignant_faults): the
    accepted configurations of exactly `weight` faults among `nb` locations whose class byte has a bit of the call's `select`, over
    the rank `ranges` ((first_rank, count) pairs, ascending and disjoint).  `records` is the (found, 2) uint64 array of
    include/gf2hip.h "malignant fault sets", sorted by (rank, kinds code); `class_names` names the bits of the class byte from bit 0
    ('accepted') up.  ranks, kind_codes and classes are its columns.  The object and its arrays are read-only."""

    def __init__(self, nb, weight, records, class_names, ranges=None):
        records = np.array(records, dtype=np.uint64).reshape(-1, _native.FAULT_RECORD_WORDS)
        nb, weight = int(nb), int(weight)
        if not 0 <= weight <= min(nb, _native.ENUMERATE_MAX_WEIGHT):
            raise ValueError("a fault list's weight lies in [0, min(nb, %d)]" % _native.ENUMERATE_MAX_WEIGHT)
        class_names = tuple(class_names)
        if not class_names or class_names[0] != 'accepted' or len(class_names) > 8:
            raise ValueError("the class byte's bit 0 is 'accepted', and it has at most 8 bits")
        total = math.comb(nb, weight)
        ranges = ((0, total),) if ranges is None else tuple((int(f), int(n)) for f, n in ranges)
        if any(f < 0 or n < 0 or f + n > total for f, n in ranges) or any(a[0] + a[1] > b[0] for a, b in zip(ranges[:-1], ranges[1:])):
            raise ValueError("the rank ranges of a fault list are ascending, disjoint and within [0, C(nb, weight))")
        ranks = records[:, 0].copy()
        codes = (records[:, 1] & np.uint64(0xFFFF)).astype(np.int64)
        classes = ((records[:, 1] >> np.uint64(32)) & np.uint64(0xFF)).astype(np.uint8)
        if len(records):
            ordered = (ranks[1:] > ranks[:-1]) | ((ranks[1:] == ranks[:-1]) & (codes[1:] > codes[:-1]))
            covered = np.zeros(len(records), dtype=bool)
            for f, n in ranges:
                covered |= (ranks >= np.uint64(f)) & (ranks < np.uint64(f + n))
            if (not covered.all() or int(codes.max()) >= 3**weight or not ordered.all()
                    or (records[:, 1] & ~np.uint64(0xFF0000FFFF)).any() or not (classes & 1).all()):
                raise ValueError("records must be accepted configurations of the ranges, sorted by (rank, kinds code), stray bits zero")
        for arr in (records, ranks, codes, classes):
            arr.setflags(write=False)
        for name, value in (('nb', nb), ('weight', weight), ('records', records), ('class_names', class_names), ('ranges', ranges),
                            ('ranks', ranks), ('kind_codes', codes), ('classes', classes)):
            object.__setattr__(self, name, value)

    def __setattr__(self, name, value):
        raise AttributeError("a FaultList is immutable")

    def __len__(self):
        return len(self.records)

    def __add__(self, other):
        """The list over both lists' ranges: `other`'s ranges lie above this one's; the records are concatenated in order."""
        if not isinstance(other, FaultList):
            return NotImplemented
        if (self.nb, self.weight, self.class_names) != (other.nb, other.weight, other.class_names):
            raise ValueError("only lists of one (nb, weight) and one gadget's classes concatenate")
        return FaultList(self.nb, self.weight, np.concatenate((self.records, other.records)), self.class_names, self.ranges + other.ranges)

    def _hit(self, mask):
        return np.ones(len(self), dtype=bool) if mask is None else (self.classes & np.uint8(int(mask) & 0xFF)) != 0

    def locations(self):
        """(found, weight) int64: the locations of every record, ascending along a row -- its rank unranked in the combinatorial
        number system (pick k is the largest s with C(s, k + 1) <= what is left of the rank), on the host."""
        out = np.zeros((len(self), self.weight), dtype=np.int64)
        left = self.ranks.copy()
        top = (1 << 63) - 1                                          # ranks lie below 2^63; larger binomials only need to compare above
        for k in range(self.weight, 0, -1):
            table = np.array([min(math.comb(s, k), top) for s in range(self.nb + 1)], dtype=np.uint64)
            pick = np.searchsorted(table, left, side='right') - 1
            out[:, k - 1] = pick
            left = left - table[pick]
        return out

    def kinds(self):
        """(found, weight) uint8: the kind (0 X, 1 Y, 2 Z) of every pick, in the order of locations()."""
        codes = self.kind_codes.copy()
        out = np.zeros((len(self), self.weight), dtype=np.uint8)
        for j in range(self.weight):
            out[:, j] = codes % 3
            codes //= 3
        return out

    def composition_counts(self, mask=None):
        """(weight + 1, weight + 1) int64 [n_x][n_y]: the records whose class byte has a bit of `mask` (None: all), per kind
        composition -- PostSelectedStrata's counts of the matching indicator field."""
        kinds = self.kinds()[self._hit(mask)]
        out = np.zeros((self.weight + 1, self.weight + 1), dtype=np.int64)
        np.add.at(out, ((kinds == 0).sum(axis=1), (kinds == 1).sum(axis=1)), 1)
        return out

    def location_counts(self, mask=None):
        """(nb,) int64: in how many of the listed sets (with a class bit of `mask`; None: all) each location takes part."""
        return np.bincount(self.locations()[self._hit(mask)].reshape(-1), minlength=self.nb).astype(np.int64)

    def coefficient(self, kinds=(1, 1, 1), mask=None):
        """sum over the records (with a class bit of `mask`) of prod_picks k_kind / s^weight as a fractions.Fraction (a float when
        the kinds are not rational): PostSelectedStrata.coefficients' A_w of the matching indicator field when the list is whole."""
        kinds = _kind_ratio(kinds)
        exact = all(isinstance(k, numbers.Rational) for k in kinds)
        k_x, k_y, k_z = (_fractions.Fraction(k) for k in kinds) if exact else (float(k) for k in kinds)
        w, counts = self.weight, self.composition_counts(mask)
        total = _fractions.Fraction(0) if exact else 0.0
        for n_x in range(w + 1):
            for n_y in range(w + 1 - n_x):
                if counts[n_x, n_y]:
                    total += int(counts[n_x, n_y]) * k_x**n_x * k_y**n_y * k_z**(w - n_x - n_y)
        return total / (k_x + k_y + k_z)**w


FAULT_LIST_FIRST_CAPACITY = 1 << 16                                  # records of malignant_faults' first call
FAULT_LIST_MAX_RECORDS = 1 << 26                                     # ... and the most it returns


def malignant_faults(nb, weight, class_names, select, first_rank, count, max_configurations, what, run):
    """What ECCircuit.malignant_faults and FTProgram.malignant_faults share: the request checked as the exact strata's
    (circuit_noise.gadget_enumerate_request), run(w, first, count, select, capacity) -> (found, records or None) called with
    FAULT_LIST_FIRST_CAPACITY records and, if they do not hold the list, once more with exactly `found`."""
    from . import circuit_noise
    (weight,), (first,), (count,) = circuit_noise.gadget_enumerate_request(nb, [int(weight)], first_rank, count, max_configurations, what)
    select = int(select)
    if select <= 0 or select >> len(class_names):
        raise ValueError("select is a non-empty subset of the class bits 0x%x (%s)" % ((1 << len(class_names)) - 1, ', '.join(class_names)))
    found, records = run(weight, first, count, select, FAULT_LIST_FIRST_CAPACITY)
    if records is None:
        if found > FAULT_LIST_MAX_RECORDS:
            raise ValueError("%d fault configurations to list, more than %d (2^26): choose a narrower select or a smaller rank range"
                             % (found, FAULT_LIST_MAX_RECORDS))
        found, records = run(weight, first, count, select, found)
    return FaultList(nb, weight, records, class_names, [(first, count)])


# ---- malignant fault sets under gate-level faults (DESIGN.md section 5e "Malignant fault sets under gate-level faults") ------------

def _unrank_subsets(n, k, ranks):
    """(len(ranks), k) int64: the subsets of [0, n) of the given ranks in the combinatorial number system, ascending along a row
    (FaultList.locations' exact-binomial search)."""
    out = np.zeros((len(ranks), k), dtype=np.int64)
    left = np.array(ranks, dtype=np.uint64)
    top = (1 << 63) - 1                                              # ranks lie below 2^63; larger binomials only need to compare above
    for j in range(k, 0, -1):
        table = np.array([min(math.comb(s, j), top) for s in range(n + 1)], dtype=np.uint64)
        pick = np.searchsorted(table, left, side='right') - 1
        out[:, j - 1] = pick
        left = left - table[pick]
    return out


class GateFaultList(object):
    """The listed configurations of faulty gates of a post-selected gadget (ec_noise.ECCircuit / ft_noise.FTProgram
    .malignant_gate_faults): the accepted configurations of exactly `weight` faulty gates, `b` of them CNOTs, among `n1` one-operand
    sites and `n2` CNOT sites whose class byte has a bit of the call's `select`, over the rank `ranges` ((first_rank, count) pairs,
    ascending and disjoint, rank = r_s + C(n1, weight - b) r_c).  `records` is the (found, 2) uint64 array of include/gf2hip.h
    "malignant fault sets under gate-level faults", sorted by (rank, kind masks); `class_names` names the bits of the class byte from
    bit 0 ('accepted') up.  ranks, kind_masks (the 16 bits of nibbles) and classes are its columns.  The object and its arrays are
    read-only."""

    def __init__(self, n1, n2, weight, b, records, class_names, ranges=None):
        records = np.array(records, dtype=np.uint64).reshape(-1, _native.FAULT_RECORD_WORDS)
        n1, n2, weight, b = int(n1), int(n2), int(weight), int(b)
        if n1 < 0 or n2 < 0 or not 0 <= b <= weight <= _native.GATE_ENUMERATE_MAX_WEIGHT:
            raise ValueError("a gate-fault list has n1, n2 >= 0 sites and 0 <= b <= weight <= %d" % _native.GATE_ENUMERATE_MAX_WEIGHT)
        class_names = tuple(class_names)
        if not class_names or class_names[0] != 'accepted' or len(class_names) > 8:
            raise ValueError("the class byte's bit 0 is 'accepted', and it has at most 8 bits")
        a = weight - b
        total = math.comb(n1, a) * math.comb(n2, b)
        ranges = ((0, total),) if ranges is None else tuple((int(f), int(n)) for f, n in ranges)
        if any(f < 0 or n < 0 or f + n > total for f, n in ranges) or any(p[0] + p[1] > q[0] for p, q in zip(ranges[:-1], ranges[1:])):
            raise ValueError("the rank ranges of a gate-fault list are ascending, disjoint and within [0, C(n1, a) C(n2, b))")
        ranks = records[:, 0].copy()
        masks = (records[:, 1] & np.uint64(0xFFFF)).astype(np.int64)
        classes = ((records[:, 1] >> np.uint64(32)) & np.uint64(0xFF)).astype(np.uint8)
        if len(records):
            ordered = (ranks[1:] > ranks[:-1]) | ((ranks[1:] == ranks[:-1]) & (masks[1:] > masks[:-1]))
            covered = np.zeros(len(records), dtype=bool)
            for f, n in ranges:
                covered |= (ranks >= np.uint64(f)) & (ranks < np.uint64(f + n))
            nibbles = (masks[:, None] >> (4 * np.arange(4))) & 15
            legal = np.ones(len(records), dtype=bool)
            for j in range(4):
                top = 3 if j < a else 15 if j < weight else 0
                legal &= (nibbles[:, j] <= top) & ((nibbles[:, j] >= 1) | (j >= weight))
            if (not covered.all() or not legal.all() or not ordered.all() or (records[:, 1] & ~np.uint64(0xFF0000FFFF)).any()
                    or not (classes & 1).all()):
                raise ValueError("records must be accepted configurations of the ranges, sorted by (rank, kind masks), stray bits zero")
        for arr in (records, ranks, masks, classes):
            arr.setflags(write=False)
        for name, value in (('n1', n1), ('n2', n2), ('weight', weight), ('b', b), ('records', records), ('class_names', class_names),
                            ('ranges', ranges), ('ranks', ranks), ('kind_masks', masks), ('classes', classes)):
            object.__setattr__(self, name, value)

    def __setattr__(self, name, value):
        raise AttributeError("a GateFaultList is immutable")

    def __len__(self):
        return len(self.records)

    def __add__(self, other):
        """The list over both lists' ranges: `other`'s ranges lie above this one's; the records are concatenated in order."""
        if not isinstance(other, GateFaultList):
            return NotImplemented
        if (self.n1, self.n2, self.weight, self.b, self.class_names) != (other.n1, other.n2, other.weight, other.b, other.class_names):
            raise ValueError("only lists of one (n1, n2, weight, b) and one gadget's classes concatenate")
        return GateFaultList(self.n1, self.n2, self.weight, self.b, np.concatenate((self.records, other.records)), self.class_names,
                             self.ranges + other.ranges)

    def _hit(self, mask):
        return np.ones(len(self), dtype=bool) if mask is None else (self.classes & np.uint8(int(mask) & 0xFF)) != 0

    def sites(self):
        """(found, weight) int64: the sites of every record's picks -- the weight - b one-operand sites first, then the b CNOT sites
        (n1 + their index among the CNOTs), each part ascending: the two parts of its rank unranked on the host."""
        a = self.weight - self.b
        c1 = np.uint64(math.comb(self.n1, a))
        out = np.zeros((len(self), self.weight), dtype=np.int64)
        if len(self):
            out[:, :a] = _unrank_subsets(self.n1, a, self.ranks % c1)
            out[:, a:] = self.n1 + _unrank_subsets(self.n2, self.b, self.ranks // c1)
        return out

    def gates(self, site_gate):
        """sites() mapped to gate indices by `site_gate` (Gadget.gate_sites()[3])."""
        site_gate = np.asarray(site_gate, dtype=np.int64).reshape(-1)
        if len(site_gate) != self.n1 + self.n2:
            raise ValueError("site_gate has one gate index per site: %d, not %d" % (self.n1 + self.n2, len(site_gate)))
        return site_gate[self.sites()]

    def kinds(self):
        """(found, weight) uint8: the kind mask kappa of every pick, in the order of sites(): 1 X, 2 Z, 3 Y on a one-operand gate;
        on a CNOT bits 0, 1 the control's X and Z components and bits 2, 3 the target's."""
        return ((self.kind_masks[:, None] >> (4 * np.arange(self.weight, dtype=np.int64))) & 15).astype(np.uint8).reshape(len(self), self.weight)

    def two_operand(self):
        """(found,) int64: c, the number of CNOT picks of every record whose kind acts on both operands."""
        kappa = self.kinds()[:, self.weight - self.b:]
        return (((kappa & 3) != 0) & ((kappa >> 2) != 0)).sum(axis=1).astype(np.int64)

    def counts(self, mask=None):
        """(b + 1,) int64 [c]: the records whose class byte has a bit of `mask` (None: all) per number c of two-operand kinds --
        GateStrata.counts[weight][b][:, field] of the matching indicator field when the list is whole."""
        return np.bincount(self.two_operand()[self._hit(mask)], minlength=self.b + 1).astype(np.int64)

    def gate_counts(self, site_gate, mask=None):
        """(gates,) int64: in how many of the listed sets (with a class bit of `mask`; None: all) each gate takes part."""
        gates = self.gates(site_gate)[self._hit(mask)]
        return np.bincount(gates.reshape(-1), minlength=int(np.max(site_gate, initial=-1)) + 1).astype(np.int64)

    def coefficient(self, odds, mask=None):
        """sum over the records (with a class bit of `mask`) of x^(weight - b) y1^(b - c) y2^c at the odds (x, y1, y2) of
        GateStrata.depolarising_odds / independent_odds (fractions.Fraction odds give an exact result): the list's term of
        GateStrata.joint without its factor Z."""
        x, y1, y2 = odds
        return sum((int(n) * x**(self.weight - self.b) * y1**(self.b - c) * y2**c for c, n in enumerate(self.counts(mask)) if n), 0 * x)


class GateFaultLists(object):
    """The whole strata of one weight listed for every CNOT count: `lists[b]`, b = 0 .. weight, a GateFaultList each (what
    malignant_gate_faults returns for b=None).  Indexing and iteration go over b; counts, gate_counts and coefficient are the
    GateFaultList's, stacked or summed over b."""

    def __init__(self, lists):
        lists = tuple(lists)
        if not lists or any(not isinstance(l, GateFaultList) for l in lists):
            raise ValueError("one GateFaultList per CNOT count")
        head = lists[0]
        if len(lists) != head.weight + 1 or any((l.n1, l.n2, l.weight, l.b, l.class_names) != (head.n1, head.n2, head.weight, b, head.class_names)
                                                for b, l in enumerate(lists)):
            raise ValueError("the lists are those of b = 0 .. weight of one (n1, n2, weight) and one gadget's classes")
        self.lists = lists
        self.n1, self.n2, self.weight, self.class_names = head.n1, head.n2, head.weight, head.class_names

    def __getitem__(self, b):
        return self.lists[b]

    def __iter__(self):
        return iter(self.lists)

    def __len__(self):
        """The records of all the lists."""
        return sum(len(l) for l in self.lists)

    def counts(self, mask=None):
        """(weight + 1, weight + 1) int64 [b][c]: GateStrata.counts[weight][:, :, field] of the matching indicator field."""
        out = np.zeros((self.weight + 1, self.weight + 1), dtype=np.int64)
        for b, l in enumerate(self.lists):
            out[b, :b + 1] = l.counts(mask)
        return out

    def gate_counts(self, site_gate, mask=None):
        return sum(l.gate_counts(site_gate, mask) for l in self.lists)

    def coefficient(self, odds, mask=None):
        return sum((l.coefficient(odds, mask) for l in self.lists), 0 * odds[0])


def malignant_gate_faults(n1, n2, weight, b, class_names, select, first_rank, count, max_configurations, what, run):
    """What ECCircuit.malignant_gate_faults and FTProgram.malignant_gate_faults share.  The request is checked as the exact gate
    strata's (circuit_noise.gate_enumerate_request's limits and budget, the size named); b=None lists the whole stratum of every b and
    takes no rank range.  run(w, b, first, count, select, capacity) -> (found, records or None) is called with
    FAULT_LIST_FIRST_CAPACITY records and, if they do not hold the list, once more with exactly `found`.  Returns a GateFaultList, or
    a GateFaultLists for b=None."""
    from . import circuit_noise
    weight = int(weight)
    if not 0 <= weight <= _native.GATE_ENUMERATE_MAX_WEIGHT:
        raise ValueError("a gate-fault stratum's weight lies in [0, %d]" % _native.GATE_ENUMERATE_MAX_WEIGHT)
    if not 1 <= n1 + 2 * n2 <= circuit_noise.MAX_LOCATIONS:
        raise ValueError("the enumeration needs 1 <= L <= %d (2^20) fault locations, the %s has %d" % (circuit_noise.MAX_LOCATIONS, what, n1 + 2 * n2))
    select = int(select)
    if select <= 0 or select >> len(class_names):
        raise ValueError("select is a non-empty subset of the class bits 0x%x (%s)" % ((1 << len(class_names)) - 1, ', '.join(class_names)))
    subsets = lambda k: math.comb(n1, weight - k) * math.comb(n2, k)
    if b is None:
        if not (first_rank is None or int(first_rank) == 0) or count is not None:
            raise ValueError("b=None lists whole strata: a rank range needs one b")
        requests = [(k, 0, subsets(k)) for k in range(weight + 1)]
    else:
        b = int(b)
        if not 0 <= b <= weight:
            raise ValueError("%d CNOT picks outside [0, weight = %d]" % (b, weight))
        first = 0 if first_rank is None else int(first_rank)
        n = subsets(b) - first if count is None else int(count)
        if first < 0 or n < 0 or first + n > subsets(b):
            raise ValueError("ranks [%d, %d + %d) leave the range [0, C(%d, %d) C(%d, %d) = %d)" % (first, first, n, n1, weight - b, n2, b, subsets(b)))
        requests = [(b, first, n)]
    size = sum(n * 3**(weight - k) * 15**k for k, _, n in requests)
    budget = circuit_noise.ENUMERATE_BUDGET if max_configurations is None else int(max_configurations)
    if size > budget:
        raise ValueError("%d gate-fault configurations to enumerate, more than max_configurations = %d" % (size, budget))
    lists = []
    for k, first, n in requests:
        found, records = run(weight, k, first, n, select, FAULT_LIST_FIRST_CAPACITY)
        if records is None:
            if found > FAULT_LIST_MAX_RECORDS:
                raise ValueError("%d fault configurations to list, more than %d (2^26): choose a narrower select or a smaller rank range"
                                 % (found, FAULT_LIST_MAX_RECORDS))
            found, records = run(weight, k, first, n, select, found)
        lists.append(GateFaultList(n1, n2, weight, k, records, class_names, [(first, n)]))
    return GateFaultLists(lists) if b is None else lists[0]


# ---- sampled strata of a post-selected gadget (DESIGN.md "Sampled strata of the cycle", "Sampled strata of the measurement") --------

# MergedPostSelectedStrata.rate's result: the conditional rate lies in [lower, upper] up to the statistical error `stderr` of `estimate`.
PostSelectedRate = collections.namedtuple('PostSelectedRate', ('estimate', 'stderr', 'lower', 'upper'))


class SampledPostSelectedStrata(object):
    """Tallies of a stratified run of a post-selected gadget (ec_noise.ECCircuit.strata / ft_noise.FTProgram.strata) over `nb`
    positions: `weights` (nstrata, distinct), `samples` (N_w per stratum), `counts` (nstrata x F in the order of `fields`, field 0
    'accepted', every other field among accepted samples) and the `kinds` the strata were drawn with.  joint, acceptance and rate are
    MergedPostSelectedStrata's over these strata alone; PostSelectedStrata.merged adds exact strata."""

    SUM_FIELDS = PostSelectedStrata.SUM_FIELDS

    def __init__(self, nb, weights, samples, counts, fields, kinds=(1, 1, 1)):
        self.nb = int(nb)
        self.fields = tuple(fields)
        if not self.fields or self.fields[0] != 'accepted':
            raise ValueError("the first field of a post-selected tally is 'accepted'")
        self.weights = np.asarray(weights, dtype=np.int64).reshape(-1).copy()
        self.samples = np.asarray(samples, dtype=np.int64).reshape(-1).copy()
        self.counts = np.asarray(counts, dtype=np.uint64).reshape(len(self.weights), len(self.fields)).copy()
        self.kinds = _kind_ratio(tuple(float(k) for k in kinds))
        if self.samples.shape != self.weights.shape:
            raise ValueError("one sample count per stratum")
        if len(set(self.weights.tolist())) != len(self.weights):
            raise ValueError("the weights of the strata must be distinct")
        if len(self.weights) and (self.weights.min() < 0 or self.weights.max() > self.nb):
            raise ValueError("a stratum's weight lies in [0, nb]")
        if self.samples.size and self.samples.min() < 0:
            raise ValueError("negative sample count")

    def _column(self, field):
        if field not in self.fields:
            raise ValueError("no field %r (the fields are %s)" % (field, ', '.join(self.fields)))
        return self.fields.index(field)

    def fractions(self, field='accepted'):
        """counts / samples per stratum (0 where a stratum has no samples): the fraction of ALL samples that are accepted and
        carry `field`."""
        col = self.counts[:, self._column(field)].astype(np.float64)
        return np.divide(col, self.samples, out=np.zeros(len(col)), where=self.samples > 0)

    def _alone(self):
        return MergedPostSelectedStrata(None, [self], self.kinds)

    def joint(self, p_t, field='accepted'):
        return self._alone().joint(p_t, field)

    def acceptance(self, p_t):
        return self._alone().acceptance(p_t)

    def rate(self, p_t, field='wrong'):
        return self._alone().rate(p_t, field)

    def as_dicts(self):
        return [dict(zip(self.fields, (int(v) for v in row)), weight=int(w), samples=int(n))
                for w, n, row in zip(self.weights, self.samples, self.counts)]


class MergedPostSelectedStrata(object):
    """Exact and sampled strata of one post-selected gadget together: the exact stratum where there is one (no variance, and the
    weight counts as covered), the sampled estimate elsewhere.  `exact` is a PostSelectedStrata or None, `sampled` a list of
    SampledPostSelectedStrata over the same nb positions and fields, all drawn with one kind ratio (that of `kinds`, when given),
    which is then the ratio of the exact coefficients too; no weight may be sampled twice.

    With B_w = binomial_weights(nb, p_t)[w], a_w the fraction of stratum w that is accepted and n_w the fraction accepted with the
    field (for an exact stratum A_w / C(nb, w)):  N = sum_w B_w n_w,  D = sum_w B_w a_w,  T = the mass of the weights neither sampled
    nor enumerated."""

    def __init__(self, exact, sampled, kinds=None):
        self.exact, self.sampled = exact, list(sampled)
        if exact is None and not self.sampled:
            raise ValueError("no strata at all")
        first = exact if exact is not None else self.sampled[0]
        self.nb, self.fields = first.nb, first.fields
        if kinds is None:
            if not self.sampled:
                raise ValueError("kinds are needed when there are no sampled strata")
            kinds = self.sampled[0].kinds
        self.kinds = _kind_ratio(kinds)
        seen = set()
        for part in self.sampled:
            if part.nb != self.nb:
                raise ValueError("sampled strata over %d positions, the others over %d" % (part.nb, self.nb))
            if part.fields != self.fields:
                raise ValueError("sampled strata with fields %r, the others with %r" % (part.fields, self.fields))
            if not _same_ratio(part.kinds, self.kinds):
                raise ValueError("sampled strata drawn with kinds %r do not match %r" % (part.kinds, self.kinds))
            live = set(part.weights[part.samples > 0].tolist())
            if live & seen:
                raise ValueError("two sampled strata of one weight")
            seen |= live
        self.weights = np.array(sorted(set(exact.weights if exact is not None else ()) | seen), dtype=np.int64)

    def _column(self, field):
        if field not in self.fields:
            raise ValueError("no field %r (the fields are %s)" % (field, ', '.join(self.fields)))
        return self.fields.index(field)

    def _parts(self, field):
        """weight -> (n_w, a_w, N_w), N_w = 0 for an exact stratum."""
        self._column(field)
        out = {}
        for part in self.sampled:
            for w, n, f, a in zip(part.weights.tolist(), part.samples.tolist(), part.fractions(field), part.fractions('accepted')):
                if n > 0:
                    out[w] = (float(f), float(a), n)
        if self.exact is not None:
            for w, f, a in zip(self.exact.weights, self.exact.coefficients(self.kinds, field), self.exact.coefficients(self.kinds, 'accepted')):
                c = math.comb(self.nb, w)
                out[w] = (float(f / c), float(a / c), 0)
        return out

    def _missing_mass(self, b_all):
        have = np.zeros(self.nb + 1, dtype=bool)
        have[self.weights] = True
        return math.fsum(b_all[~have])

    def joint(self, p_t, field='accepted'):
        """P(accepted and field) at total fault probability p_t per position over the covered weights: sum_w B_w n_w."""
        b_all = binomial_weights(self.nb, p_t)
        return math.fsum(b_all[w] * f for w, (f, a, n) in self._parts(field).items())

    def acceptance(self, p_t):
        """(D, D + T): the probability that an attempt is accepted lies between them (up to the sampling error of D)."""
        b_all = binomial_weights(self.nb, p_t)
        d = math.fsum(b_all[w] * a for w, (f, a, n) in self._parts('accepted').items())
        return d, d + self._missing_mass(b_all)

    def rate(self, p_t, field='wrong'):
        """The conditional rate P(field | accepted) of an indicator field as PostSelectedRate(estimate, stderr, lower, upper):
        estimate R = N / D; lower = N / (D + T) and upper = (N + T) / (D + T) as PostSelectedStrata.rate defines them; stderr the
        delta-method error of the ratio,  (1 / D) sqrt(sum over sampled w of B_w^2 [n_w (1 - R)^2 + (a_w - n_w) R^2 - (n_w - R a_w)^2]
        / N_w):  a sample of stratum w contributes x - R y with (x, y) = (1, 1), (0, 1) or (0, 0) -- an indicator field is a subset of
        `accepted` -- whose variance is the bracket."""
        if field in PostSelectedStrata.SUM_FIELDS:
            raise ValueError("rate() is defined for indicator fields; %r is a sum" % (field,))
        b_all = binomial_weights(self.nb, p_t)
        parts = self._parts(field)
        n_tot = math.fsum(b_all[w] * f for w, (f, a, n) in parts.items())
        d = math.fsum(b_all[w] * a for w, (f, a, n) in parts.items())
        t = self._missing_mass(b_all)
        if not d > 0:
            raise ValueError("no accepted sample or configuration among the covered weights at p_t = %r" % (p_t,))
        r = n_tot / d
        var = math.fsum(b_all[w]**2 * (f * (1.0 - r)**2 + (a - f) * r**2 - (f - r * a)**2) / n for w, (f, a, n) in parts.items() if n > 0)
        return PostSelectedRate(r, math.sqrt(max(var, 0.0)) / d, n_tot / (d + t), (n_tot + t) / (d + t))


def host_strata_run(effects, tally, nfields, seed, chunk=1 << 18):
    """The `run` of gadget_strata_local on the host: gf2_stratum_outcomes_host's words, `chunk` samples at a time, handed to `tally`
    (words -> the gadget's counts; _native.ec_tally_host / ft_tally_host with the gadget's arguments)."""
    def run(first, weights, samples, kinds):
        out = np.zeros((len(weights), nfields), dtype=np.uint64)
        for s, (w, count) in enumerate(zip(weights, np.asarray(samples).tolist())):
            for done in range(0, int(count), chunk):
                now = min(chunk, int(count) - done)
                out[s] += tally(_native.stratum_outcomes_host(effects, w, now, kinds, seed, int(first) + done))
        return out
    return run


def gadget_strata_local(nb, fields, weights, samples, kinds, first_sample, run):
    """What ECCircuit.strata and FTProgram.strata share: the request checked and grouped as strata_local groups it (one native call
    per distinct first sample), `run(first, weights, samples, kinds)` returning the (nstrata, F) counts of a call."""
    weights, samples, firsts, kinds = _strata_request(weights, samples, kinds, first_sample)
    top = min(int(nb), _native.CIRCUIT_STRATUM_MAX_WEIGHT)
    if any(w < 0 or w > top for w in weights):
        raise ValueError("a stratum's weight lies in [0, min(L = %d, %d)]" % (int(nb), _native.CIRCUIT_STRATUM_MAX_WEIGHT))
    if firsts.size and firsts.min() < 0:
        raise ValueError("negative first sample")
    counts = np.zeros((len(weights), len(fields)), dtype=np.uint64)
    for first, rows in _strata_calls(firsts):
        counts[rows] = run(int(first), [weights[s] for s in rows], samples[rows], kinds)
    return SampledPostSelectedStrata(nb, weights, samples, counts, fields, kinds)


def gadget_strata_sharded(gadget, weights, samples, kinds=(1, 1, 1), seed=0, first_sample=0, group=None, local_fn=None):
    """Sampled strata of an ec_noise.ECCircuit or an ft_noise.FTProgram over the ranks of a process group: every stratum's sample
    range is cut by shard_range, this rank runs its part, and one all-reduce sums the nstrata x F counts.  `local_fn(gadget, weights,
    samples, kinds=, seed=, first_sample=)` replaces gadget.strata (the CPU tests pass the host statement).  Returns a
    SampledPostSelectedStrata with the whole sample counts."""
    rank, world = _rank_world(group)
    weights, samples, firsts, kinds = _strata_request(weights, samples, kinds, first_sample)
    shards = [shard_range(first, count, rank, world) for first, count in zip(firsts.tolist(), samples.tolist())]
    fn = local_fn or (lambda g, ws, ns, kinds, seed, first_sample: g.strata(ws, ns, kinds=kinds, seed=seed, first_sample=first_sample))
    part = fn(gadget, weights, [mine for _, mine in shards], kinds=kinds, seed=seed, first_sample=[start for start, _ in shards])
    total, = all_reduce_histograms([part.counts.reshape(-1)], group=group)
    return SampledPostSelectedStrata(part.nb, weights, samples, total, part.fields, kinds)


# ---- sampled strata under gate-level faults (DESIGN.md section 5e "Sampled strata under gate-level faults") ------------------------

GATE_STRATA_ROWS = _native.GATE_STRATUM_MAX_WEIGHT + 1


class SampledGateStrata(object):
    """Tallies of a stratified run of a post-selected gadget under gate-level faults (ec_noise.ECCircuit.gate_strata /
    ft_noise.FTProgram.gate_strata) with `n1` one-operand gates and `n2` CNOTs: `strata` (nstrata rows (a, b), distinct), `samples`
    (N per stratum), `counts` (nstrata x 17 x F, [stratum][c][field] with c the number of two-operand kinds, field 0 'accepted',
    every other field among accepted samples, the rows c > b zero).  counts[s][c] / N estimates the exact strata's
    counts[a + b][b][c] / (C(n1, a) C(n2, b) 3^a 15^b).  joint, acceptance and rate are MergedGateStrata's over these strata alone;
    GateStrata.merged adds exact strata."""

    SUM_FIELDS = PostSelectedStrata.SUM_FIELDS

    def __init__(self, n1, n2, strata, samples, counts, fields):
        self.n1, self.n2 = int(n1), int(n2)
        self.fields = tuple(fields)
        if not self.fields or self.fields[0] != 'accepted':
            raise ValueError("the first field of a post-selected tally is 'accepted'")
        self.strata = np.asarray(strata, dtype=np.int64).reshape(-1, 2).copy()
        self.samples = np.asarray(samples, dtype=np.int64).reshape(-1).copy()
        self.counts = np.asarray(counts, dtype=np.uint64).reshape(len(self.strata), GATE_STRATA_ROWS, len(self.fields)).copy()
        if self.samples.shape != (len(self.strata),):
            raise ValueError("one sample count per stratum")
        if len(set(map(tuple, self.strata.tolist()))) != len(self.strata):
            raise ValueError("the strata (a, b) must be distinct")
        for a, b in self.strata.tolist():
            if not (0 <= a <= self.n1 and 0 <= b <= self.n2 and a + b <= _native.GATE_STRATUM_MAX_WEIGHT):
                raise ValueError("a stratum (a, b) needs 0 <= a <= n1 = %d, 0 <= b <= n2 = %d and a + b <= %d, got (%d, %d)"
                                 % (self.n1, self.n2, _native.GATE_STRATUM_MAX_WEIGHT, a, b))
        if self.samples.size and self.samples.min() < 0:
            raise ValueError("negative sample count")

    def _column(self, field):
        if field not in self.fields:
            raise ValueError("no field %r (the fields are %s)" % (field, ', '.join(self.fields)))
        return self.fields.index(field)

    def fractions(self, field='accepted'):
        """counts / samples per stratum and class, (nstrata, 17): the fraction of ALL samples of the stratum that have c two-operand
        kinds, are accepted and carry `field` (0 where a stratum has no samples)."""
        col = self.counts[:, :, self._column(field)].astype(np.float64)
        n = self.samples[:, None]
        return np.divide(col, n, out=np.zeros_like(col), where=n > 0)

    def _alone(self):
        return MergedGateStrata(None, [self])

    def joint(self, odds, field='accepted'):
        return self._alone().joint(odds, field)

    def acceptance(self, odds):
        return self._alone().acceptance(odds)

    def rate(self, odds, field='wrong'):
        return self._alone().rate(odds, field)

    def as_dicts(self):
        return [dict(zip(self.fields, (int(v) for v in rows.sum(axis=0))), a=int(a), b=int(b), samples=int(n))
                for (a, b), n, rows in zip(self.strata.tolist(), self.samples, self.counts)]


class MergedGateStrata(object):
    """Exact and sampled strata of one post-selected gadget under gate-level faults together.  `exact` is a GateStrata or None,
    `sampled` a list of SampledGateStrata over the same (n1, n2) and fields; no stratum may be sampled twice.  An exact weight w
    replaces every sampled (a, b) with a + b = w (no variance) and covers its whole anti-diagonal.

    At the odds (x, y1, y2) a sampled stratum (a, b) carries, per class c, the weight
    omega = Z x^a y1^(b - c) y2^c C(n1, a) C(n2, b) 3^a 15^b with Z = (1 + 3 x)^-n1 (1 + 6 y1 + 9 y2)^-n2, and with phi the sampled
    fraction count / N:  N = sum omega phi[field],  D = sum omega phi[accepted],  T = 1 - sum over the covered (a, b) of
    P(A = a) P(B = b), A ~ Bin(n1, 3 x / (1 + 3 x)), B ~ Bin(n2, (6 y1 + 9 y2) / (1 + 6 y1 + 9 y2)).  A sampled stratum with nothing
    accepted contributes nothing and counts as covered."""

    def __init__(self, exact, sampled):
        self.exact, self.sampled = exact, list(sampled)
        if exact is None and not self.sampled:
            raise ValueError("no strata at all")
        first = exact if exact is not None else self.sampled[0]
        self.n1, self.n2, self.fields = first.n1, first.n2, first.fields
        self.exact_weights = sorted(exact.weights) if exact is not None else []
        seen = set()
        for part in self.sampled:
            if (part.n1, part.n2) != (self.n1, self.n2):
                raise ValueError("sampled strata over (n1, n2) = (%d, %d), the others over (%d, %d)" % (part.n1, part.n2, self.n1, self.n2))
            if part.fields != self.fields:
                raise ValueError("sampled strata with fields %r, the others with %r" % (part.fields, self.fields))
            live = set(tuple(s) for s, n in zip(part.strata.tolist(), part.samples.tolist()) if n > 0)
            if live & seen:
                raise ValueError("a stratum (a, b) is sampled twice: %r" % (sorted(live & seen),))
            seen |= live
        self.strata = sorted(s for s in seen if s[0] + s[1] not in self.exact_weights)   # the sampled strata that are used

    def _column(self, field):
        if field not in self.fields:
            raise ValueError("no field %r (the fields are %s)" % (field, ', '.join(self.fields)))
        return self.fields.index(field)

    @staticmethod
    def _odds(odds):
        x, y1, y2 = (float(v) for v in odds)
        if min(x, y1, y2) < 0.0:
            raise ValueError("odds are not negative")
        return x, y1, y2

    def _omega(self, odds, a, b):
        """omega_{a, b, c} for c = 0 .. b (log space; 0 where an odd with a positive exponent is 0)."""
        x, y1, y2 = odds
        log_z = -self.n1 * math.log1p(3.0 * x) - self.n2 * math.log1p(6.0 * y1 + 9.0 * y2)
        log_n = (math.lgamma(self.n1 + 1) - math.lgamma(a + 1) - math.lgamma(self.n1 - a + 1) + math.lgamma(self.n2 + 1)
                 - math.lgamma(b + 1) - math.lgamma(self.n2 - b + 1) + a * math.log(3.0) + b * math.log(15.0))
        out = np.zeros(b + 1)
        for c in range(b + 1):
            powers = ((a, x), (b - c, y1), (c, y2))
            if any(e and not v for e, v in powers):
                continue
            out[c] = math.exp(log_z + log_n + sum(e * math.log(v) for e, v in powers if e))
        return out

    def _sampled_parts(self, field):
        """(a, b) -> (field counts[c], accepted counts[c], N) of every sampled stratum that is used, c = 0 .. b."""
        col = self._column(field)
        out = {}
        for part in self.sampled:
            for (a, b), n, rows in zip(part.strata.tolist(), part.samples.tolist(), part.counts):
                if n > 0 and (a, b) in self.strata:
                    out[(a, b)] = (rows[:b + 1, col].astype(np.float64), rows[:b + 1, 0].astype(np.float64), n)
        return out

    def _sums(self, odds, field):
        """(N, D): the exact weights' joint probabilities plus sum omega phi over the sampled strata that are used."""
        n_tot = [self.exact.joint(odds, field)] if self.exact is not None else []
        d_tot = [self.exact.joint(odds, 'accepted')] if self.exact is not None else []
        for (a, b), (f, acc, n) in self._sampled_parts(field).items():
            omega = self._omega(odds, a, b)
            n_tot.append(float(np.dot(omega, f)) / n)
            d_tot.append(float(np.dot(omega, acc)) / n)
        return math.fsum(n_tot), math.fsum(d_tot)

    def joint(self, odds, field='accepted'):
        """P(accepted and field) at the odds (x, y1, y2) over the covered strata."""
        odds = self._odds(odds)
        self._column(field)
        return self._sums(odds, field)[0]

    def _missing_mass(self, odds):
        """T: the probability that (A, B) is not a covered stratum.  Whole weights through GateStrata._missing_mass' sum of two
        binomials; a weight with sampled cells directly, cell by cell, so that nothing is subtracted."""
        x, y1, y2 = odds
        q_1, q_2 = 3.0 * x / (1.0 + 3.0 * x), (6.0 * y1 + 9.0 * y2) / (1.0 + 6.0 * y1 + 9.0 * y2)
        p_a, p_b = binomial_weights(self.n1, q_1), binomial_weights(self.n2, q_2)
        total = np.convolve(p_a, p_b)
        have = np.zeros(len(total), dtype=bool)
        have[self.exact_weights] = True
        cells = {}
        for a, b in self.strata:
            cells.setdefault(a + b, set()).add(a)
        terms = []
        for w, sampled_a in cells.items():
            have[w] = True
            terms.extend(float(p_a[a] * p_b[w - a]) for a in range(max(0, w - self.n2), min(self.n1, w) + 1) if a not in sampled_a)
        terms.extend(total[~have].tolist())
        return math.fsum(terms)

    def acceptance(self, odds):
        """(D, D + T): the probability that an attempt is accepted lies between them (up to the sampling error of D)."""
        odds = self._odds(odds)
        d = self._sums(odds, 'accepted')[1]
        return d, d + self._missing_mass(odds)

    def rate(self, odds, field='wrong'):
        """The conditional rate P(field | accepted) of an indicator field as PostSelectedRate(estimate, stderr, lower, upper):
        estimate R = N / D, lower = N / (D + T), upper = (N + T) / (D + T), and stderr by the delta method: a sample of stratum
        (a, b) with class c contributes u = omega_{a,b,c} (1[field] - R 1[accepted]), and
        stderr = (1 / D) sqrt(sum over the sampled strata of (E[u^2] - E[u]^2) / N_{a,b}), the expectations over the stratum's own
        samples.  With y1 = y2 and one sampled stratum this is sqrt(R (1 - R) / (N a)), a the accepted fraction."""
        if field in PostSelectedStrata.SUM_FIELDS:
            raise ValueError("rate() is defined for indicator fields; %r is a sum" % (field,))
        odds = self._odds(odds)
        self._column(field)
        n_tot, d = self._sums(odds, field)
        t = self._missing_mass(odds)
        if not d > 0:
            raise ValueError("no accepted sample or configuration among the covered strata at the odds %r" % (odds,))
        r = n_tot / d
        var = []
        for (a, b), (f, acc, n) in self._sampled_parts(field).items():
            omega = self._omega(odds, a, b)
            mean = float(np.dot(omega, f - r * acc)) / n
            square = float(np.dot(omega**2, f * (1.0 - r)**2 + (acc - f) * r**2)) / n
            var.append((square - mean**2) / n)
        return PostSelectedRate(r, math.sqrt(max(math.fsum(var), 0.0)) / d, n_tot / (d + t), (n_tot + t) / (d + t))


def _gate_strata_request(n1, n2, strata, samples, first_sample):
    strata = [(int(a), int(b)) for a, b in np.asarray(strata, dtype=np.int64).reshape(-1, 2).tolist()]
    samples = np.broadcast_to(np.asarray(samples, dtype=np.int64), (len(strata),)).copy()
    firsts = np.broadcast_to(np.asarray(first_sample, dtype=np.int64), (len(strata),)).copy()
    top = _native.GATE_STRATUM_MAX_WEIGHT
    for a, b in strata:
        if a < 0 or b < 0 or a + b > top:
            raise ValueError("a stratum (a, b) needs a, b >= 0 and a + b <= %d faulty gates, got (%d, %d)" % (top, a, b))
        if a > n1 or b > n2:
            raise ValueError("a stratum (a, b) needs a <= n1 = %d and b <= n2 = %d, got (%d, %d)" % (n1, n2, a, b))
    if samples.size and samples.min() < 0:
        raise ValueError("negative sample count")
    if firsts.size and firsts.min() < 0:
        raise ValueError("negative first sample")
    return strata, samples, firsts


def host_gate_strata_run(effects, sites, tally, nfields, seed, chunk=1 << 18):
    """The `run` of gate_strata_local on the host: gf2_gate_stratum_outcomes_host's words and classes, `chunk` samples at a time, the
    words grouped by their class c and handed to `tally` (words -> the gadget's counts; _native.ec_tally_host / ft_tally_host)."""
    def run(first, strata, samples):
        out = np.zeros((len(strata), GATE_STRATA_ROWS, nfields), dtype=np.uint64)
        for s, ((a, b), count) in enumerate(zip(strata, np.asarray(samples).tolist())):
            for done in range(0, int(count), chunk):
                words, two = _native.gate_stratum_outcomes_host(effects, *sites, a, b, min(chunk, int(count) - done), seed, int(first) + done)
                for c in np.unique(two).tolist():
                    out[s, c] += tally(words[two == c])
        return out
    return run


def gate_strata_local(n1, n2, fields, strata, samples, first_sample, run):
    """What ECCircuit.gate_strata and FTProgram.gate_strata share: the request checked and grouped as strata_local groups it (one
    native call per distinct first sample), `run(first, strata, samples)` returning the (nstrata, 17, F) counts of a call."""
    strata, samples, firsts = _gate_strata_request(n1, n2, strata, samples, first_sample)
    counts = np.zeros((len(strata), GATE_STRATA_ROWS, len(fields)), dtype=np.uint64)
    for first, rows in _strata_calls(firsts):
        counts[rows] = run(int(first), [strata[s] for s in rows], samples[rows])
    return SampledGateStrata(n1, n2, strata, samples, counts, fields)


def gate_strata_sharded(gadget, strata, samples, seed=0, first_sample=0, group=None, local_fn=None):
    """Sampled strata under gate-level faults of an ec_noise.ECCircuit or an ft_noise.FTProgram over the ranks of a process group:
    every stratum's sample range is cut by shard_range, this rank runs its part, and one all-reduce sums the nstrata x 17 x F counts.
    `local_fn(gadget, strata, samples, seed=, first_sample=)` replaces gadget.gate_strata (the CPU tests pass the host statement).
    Returns a SampledGateStrata with the whole sample counts."""
    rank, world = _rank_world(group)
    _, n1, n2, _ = gadget.gate_sites()
    strata, samples, firsts = _gate_strata_request(n1, n2, strata, samples, first_sample)
    shards = [shard_range(first, count, rank, world) for first, count in zip(firsts.tolist(), samples.tolist())]
    fn = local_fn or (lambda g, strata, ns, seed, first_sample: g.gate_strata(strata, ns, seed=seed, first_sample=first_sample))
    part = fn(gadget, strata, [mine for _, mine in shards], seed=seed, first_sample=[start for start, _ in shards])
    total, = all_reduce_histograms([part.counts.reshape(-1)], group=group)
    return SampledGateStrata(n1, n2, strata, samples, total, part.fields)


def host_gate_counts(effects, sites, tally, nfields, num_samples, p1, p2, seed, first_sample, chunk=1 << 18):
    """The counts of the direct Monte-Carlo under gate-level faults on the host (DESIGN.md section 5e "Direct Monte-Carlo under
    gate-level faults"): gf2_gate_outcomes_host's words of samples [first_sample, first_sample + num_samples), `chunk` at a time,
    handed to `tally` (words -> the gadget's counts; _native.ec_tally_host / ft_tally_host) and summed."""
    if int(num_samples) < 0:
        raise ValueError("negative sample count")
    out = np.zeros(nfields, dtype=np.uint64)
    if int(num_samples) == 0:                                           # (the native call still checks the other arguments)
        _native.gate_outcomes_host(effects, *sites, 0, p1, p2, seed, int(first_sample), faults=False)
    for done in range(0, int(num_samples), chunk):
        words, _ = _native.gate_outcomes_host(effects, *sites, min(chunk, int(num_samples) - done), p1, p2, seed, int(first_sample) + done,
                                              faults=False)
        out += tally(words)
    return out


def gate_error_rates_sharded(gadget, num_samples, p1, p2, seed=0, first_sample=0, group=None, local_fn=None):
    """The direct Monte-Carlo under gate-level faults of an ec_noise.ECCircuit or an ft_noise.FTProgram over the ranks of a process
    group: the sample range is cut by shard_range, this rank runs its part, and one all-reduce sums the counts (counts of sample
    ranges add).  `local_fn(gadget, num_samples, p1, p2, seed=, first_sample=)` replaces gadget.gate_error_rates (the CPU tests pass
    the host statement).  Returns gate_error_rates' dict with the whole sample count."""
    rank, world = _rank_world(group)
    start, mine = shard_range(first_sample, num_samples, rank, world)
    fn = local_fn or (lambda g, n, p1, p2, seed, first_sample: g.gate_error_rates(n, p1, p2, seed=seed, first_sample=first_sample))
    part = fn(gadget, mine, p1, p2, seed=seed, first_sample=start)
    names = [name for name in part if name != 'samples']
    total, = all_reduce_histograms([np.array([part[name] for name in names], dtype=np.uint64)], group=group)
    out = {name: int(v) for name, v in zip(names, total)}
    out['samples'] = int(num_samples)
    return out


def enumerate_sharded(circuit, weights, group=None, local_fn=None):
    """The whole strata `weights` of a FaultCircuit over the ranks of a process group: every weight's rank range [0, C(L, w)) is cut
    by shard_range, this rank enumerates its part, and one all-reduce sums the counts.  `local_fn(circuit, weights, first_rank,
    count)` replaces circuit.enumerate_strata (the CPU tests pass the host statement).  Returns an ExactStrata -- or, for an
    ec_noise.ECCircuit or an ft_noise.FTProgram, whose parts are PostSelectedStrata, a PostSelectedStrata: the field count and the
    class of the result are those of the part."""
    rank, world = _rank_world(group)
    weights = [int(w) for w in np.asarray(weights).reshape(-1)]
    shards = [shard_range(0, math.comb(circuit.num_locations, w), rank, world) for w in weights]
    fn = local_fn or (lambda circ, ws, first_rank, count: circ.enumerate_strata(ws, first_rank=first_rank, count=count))
    part = fn(circuit, weights, [start for start, _ in shards], [mine for _, mine in shards])
    total, = all_reduce_histograms([np.concatenate([c.reshape(-1) for c in part.counts]) if weights else np.zeros(0, dtype=np.uint64)],
                                   group=group)
    post_selected = isinstance(part, PostSelectedStrata)
    nfields = len(part.fields) if post_selected else len(DECODE_FIELDS)
    counts, at = [], 0
    for w in weights:
        size = (w + 1) * (w + 1) * nfields
        counts.append(total[at:at + size])
        at += size
    if post_selected:
        return PostSelectedStrata(circuit.num_locations, weights, counts, part.fields)
    return ExactStrata(circuit.num_locations, weights, counts)
