"""
ORACLE -- test infrastructure only.  Exact distributions of what the Monte-Carlo entry points histogram and tally, and the
statistics that compare a histogram with them ("Distribution").  NumPy and the standard library only.

The noise is independent per qubit (or per fault location) and every outcome is a GF(2)-linear function of the error, so an
outcome's distribution is the convolution over Z_2^m of one small distribution per qubit.  Its Walsh-Hadamard transform is
the product of closed-form factors: a point mass at v transforms to (-1)^(s.v).  For one check H (r x n) and flip rate q
    P(sigma) = 2^-r  sum_s (-1)^(s.sigma) (1 - 2q)^wt(s^T H).
Nothing here samples, and nothing here is derived from the kernels: which check sees which error component comes from
css_code.py (X errors are caught by parity_check_c2, Z errors by parity_check_c1; Y is both).

Index of a joint cell (the Monte-Carlo word layout of DESIGN.md 5a, packed):
    key_x | key_z << r_2 | parity_z_op << (r_1 + r_2) | parity_x_op << (r_1 + r_2 + 1)
key_x = vec_to_int(parity_check_c2 . e_x), key_z = vec_to_int(parity_check_c1 . e_z) (row 0 = most significant bit),
parity_z_op = z_operator . e_x, parity_x_op = x_operator . e_z.
"""
import math

import numpy as np

MAX_JOINT_BITS = 22
MAX_MARGINAL_BITS = 24


# ---- transform ---------------------------------------------------------------------------------------------------------

def fwht(a):
    """In-place fast Walsh-Hadamard transform (unnormalised) of a float64 array of 2^m entries; returns it."""
    size = a.size
    if a.dtype != np.float64 or a.ndim != 1 or size < 1 or size & (size - 1):
        raise ValueError("fwht needs a one-dimensional float64 array of 2^m entries")
    h = 1
    while h < size:
        pairs = a.reshape(-1, 2, h)
        low = pairs[:, 0, :].copy()
        pairs[:, 0, :] += pairs[:, 1, :]
        np.subtract(low, pairs[:, 1, :], out=pairs[:, 1, :])
        h *= 2
    return a


def _character(value, m):
    """(-1)^(s . value) for every s in [0, 2^m): the transform of a point mass at `value`."""
    out = np.ones(1, dtype=np.float64)
    for bit in range(m):
        out = np.concatenate((out, -out if (value >> bit) & 1 else out))
    return out


def product_distribution(m, points, probs):
    """Distribution over [0, 2^m) of the XOR over locations l of an independent variable that takes points[l][k] with
    probability probs[k] and 0 otherwise.  points: (L, K) integers.  float64, exact to rounding."""
    if m > MAX_MARGINAL_BITS:
        raise ValueError("a transform of more than 2^%d cells is refused" % MAX_MARGINAL_BITS)
    points = np.asarray(points, dtype=np.int64).reshape(-1, len(probs))
    rest = 1.0 - math.fsum(probs)
    spectrum = np.ones(1 << m, dtype=np.float64)
    kinds, counts = np.unique(points, axis=0, return_counts=True) if len(points) else (points, [])
    for row, times in zip(kinds.tolist(), counts):
        factor = np.full(1 << m, rest)
        for value, p in zip(row, probs):
            if p != 0.0:
                factor += p * _character(int(value), m)
        spectrum *= factor ** int(times)
    out = fwht(spectrum)
    out /= float(1 << m)
    np.clip(out, 0.0, 1.0, out=out)
    return out


# ---- one check ---------------------------------------------------------------------------------------------------------

def _column_keys(h):
    """vec_to_int of every column of a check (row 0 = most significant bit), as Python ints."""
    h = np.asarray(h) & 1
    r = h.shape[0]
    return [sum(int(h[i, j]) << (r - 1 - i) for i in range(r)) for j in range(h.shape[1])]


def marginal(h, q):
    """The 2^r-bin distribution of vec_to_int(H . e) for independent bit flips at rate q.  hist_z follows
    marginal(parity_check_c1, p_y + p_z) and hist_x follows marginal(parity_check_c2, p_x + p_y): a Y error has both
    components, and css_code.py sends the Z component through C1's check and the X component through C2's."""
    h = np.asarray(h)
    if h.shape[0] > MAX_MARGINAL_BITS:
        raise ValueError("marginal needs r <= %d" % MAX_MARGINAL_BITS)
    return product_distribution(h.shape[0], np.array(_column_keys(h)).reshape(-1, 1), [float(q)])


def weight_projection(dist, r):
    """(r + 1) bins by population count of the key: what mode 'weight' histograms."""
    keys = np.arange(dist.size, dtype=np.int64)
    weight = np.zeros(dist.size, dtype=np.int64)
    for bit in range(r):
        weight += (keys >> bit) & 1
    return np.bincount(weight, weights=dist, minlength=r + 1)


def syndrome_weight_mean_var(h, q):
    """Exact mean and variance of wt(H . e) for checks too tall for a transform.  With lam = 1 - 2q and w_i the weight of
    row i:  E[s_i] = (1 - lam^w_i) / 2,  E[s_i s_j] = (1 - lam^w_i - lam^w_j + lam^wt(row_i ^ row_j)) / 4."""
    h = (np.asarray(h) & 1).astype(np.float32)
    lam = 1.0 - 2.0 * float(q)
    w = h.sum(axis=1).astype(np.float64)
    overlap = (h @ h.T).astype(np.float64)                       # exact: counts below 2^24
    pair_w = w[:, None] + w[None, :] - 2.0 * overlap
    a = lam ** w
    mean_i = (1.0 - a) / 2.0
    both = (1.0 - a[:, None] - a[None, :] + lam ** pair_w) / 4.0
    cov = both - mean_i[:, None] * mean_i[None, :]
    return float(mean_i.sum()), float(cov.sum())


# ---- joints ------------------------------------------------------------------------------------------------------------

class Joint(object):
    """prob: 2^(r_1 + r_2 + 2) cells in the layout of the module docstring."""

    def __init__(self, prob, r_1, r_2):
        self.prob, self.r_1, self.r_2 = prob, int(r_1), int(r_2)

    def _axes(self):
        return self.prob.reshape(2, 2, 1 << self.r_1, 1 << self.r_2)          # [parity_x_op, parity_z_op, key_z, key_x]

    def hist_x(self):
        return self._axes().sum(axis=(0, 1, 2))

    def hist_z(self):
        return self._axes().sum(axis=(0, 1, 3))


def _bits_to_key(column):
    r = len(column)
    return sum(int(column[i]) << (r - 1 - i) for i in range(r))


def code_capacity_joint(code, p_x, p_y, p_z):
    """Exact distribution over [key_x | key_z | parity_z_op | parity_x_op] of one independent Pauli error per qubit.  `code`
    has parity_check_c1 / _c2, z_operator_matrix() and x_operator_matrix() (the product's CSSCode or the oracle's)."""
    h_1, h_2 = np.asarray(code.parity_check_c1) & 1, np.asarray(code.parity_check_c2) & 1
    r_1, r_2 = h_1.shape[0], h_2.shape[0]
    m = r_1 + r_2 + 2
    if m > MAX_JOINT_BITS:
        raise ValueError("the joint needs r_1 + r_2 + 2 <= %d" % MAX_JOINT_BITS)
    z_op, x_op = np.asarray(code.z_operator_matrix())[0] & 1, np.asarray(code.x_operator_matrix())[0] & 1
    points = []
    for j in range(h_1.shape[1]):
        effect_x = _bits_to_key(h_2[:, j]) | int(z_op[j]) << (r_1 + r_2)          # the X component meets C2's check and Z_L
        effect_z = _bits_to_key(h_1[:, j]) << r_2 | int(x_op[j]) << (r_1 + r_2 + 1)
        points.append((effect_x, effect_x ^ effect_z, effect_z))
    return Joint(product_distribution(m, points, [float(p_x), float(p_y), float(p_z)]), r_1, r_2)


def pack_outcome_words(words, r_1, r_2):
    """Cell index of outcome words in the Monte-Carlo layout ([key_x: 1 word] [key_z: 1 word] [parity: 1 word], r <= 63)."""
    words = np.asarray(words, dtype=np.uint64)
    mask = lambda r: np.uint64((1 << r) - 1)
    idx = (words[..., 0] & mask(r_2)) | ((words[..., 1] & mask(r_1)) << np.uint64(r_2)) | \
        ((words[..., 2] & np.uint64(3)) << np.uint64(r_1 + r_2))
    return idx.astype(np.int64)


def circuit_joint(effects, p_x, p_y, p_z, r_1, r_2):
    """The same product over the L fault locations of an effect table of gf2_circuit_effects made for a code
    (FaultCircuit.for_code): effects[l][0] = outcome words of an X fault at location l, effects[l][1] of a Z fault."""
    effects = np.asarray(effects, dtype=np.uint64)
    if effects.ndim != 3 or effects.shape[1] != 2 or effects.shape[2] != 3:
        raise ValueError("effects must be (L, 2, 3) words: key_x, key_z, parity")
    if r_1 + r_2 + 2 > MAX_JOINT_BITS:
        raise ValueError("the joint needs r_1 + r_2 + 2 <= %d" % MAX_JOINT_BITS)
    cells = pack_outcome_words(effects, r_1, r_2)                          # (L, 2)
    assert np.array_equal(effects[..., 0] >> np.uint64(r_2), np.zeros_like(cells, dtype=np.uint64))
    points = np.stack((cells[:, 0], cells[:, 0] ^ cells[:, 1], cells[:, 1]), axis=1)
    return Joint(product_distribution(r_1 + r_2 + 2, points, [float(p_x), float(p_y), float(p_z)]), r_1, r_2)


def expected_decode_counts(joint, table_c1, table_c2, ops, num_samples=1):
    """Exact expectation and binomial variance of the five DECODE_FIELDS (logical_x, logical_z, logical_any,
    uncorrectable_x, uncorrectable_z) over `num_samples` samples.  Tables: dict vec_to_int(syndrome) -> error vector;
    ops = (x_operator, z_operator) as 0/1 vectors.  A syndrome absent from its table gets no correction and counts as
    uncorrectable (css_code.py:655-657): the flip is then the error's own parity."""
    x_op, z_op = (np.asarray(op).reshape(-1) & 1 for op in ops)

    def per_key(table, r, op):
        flip = np.zeros(1 << r, dtype=np.int64)
        miss = np.ones(1 << r, dtype=np.int64)
        for key, err in table.items():
            flip[int(key)] = int(np.dot(op, np.asarray(err).reshape(-1) & 1)) & 1
            miss[int(key)] = 0
        return flip, miss
    flip_x, miss_x = per_key(table_c2, joint.r_2, z_op)                      # X errors: C2's table, Z_L decides
    flip_z, miss_z = per_key(table_c1, joint.r_1, x_op)
    prob = joint._axes()
    parity = np.arange(2).reshape(2, 1, 1, 1)
    lx = np.broadcast_to(parity.reshape(1, 2, 1, 1) ^ flip_x.reshape(1, 1, 1, -1), prob.shape)
    lz = np.broadcast_to(parity ^ flip_z.reshape(1, 1, -1, 1), prob.shape)
    ux = np.broadcast_to(miss_x.reshape(1, 1, 1, -1), prob.shape)
    uz = np.broadcast_to(miss_z.reshape(1, 1, -1, 1), prob.shape)
    p = np.array([float((prob * ind).sum()) for ind in (lx, lz, lx | lz, ux, uz)])
    return num_samples * p, num_samples * p * (1.0 - p)


# ---- tail probabilities ------------------------------------------------------------------------------------------------

def _gamma_prefactor(a, x):
    return math.exp(a * math.log(x) - x - math.lgamma(a))


def _gamma_p_series(a, x):
    """P(a, x) by the power series (x < a + 1)."""
    term = total = 1.0 / a
    k = a
    for _ in range(10**7):
        k += 1.0
        term *= x / k
        total += term
        if term < total * 1e-17:
            break
    return total * _gamma_prefactor(a, x)


def _gamma_q_fraction(a, x):
    """Q(a, x) by Lentz's continued fraction (x >= a + 1)."""
    tiny = 1e-300
    b = x + 1.0 - a
    c = 1.0 / tiny
    d = 1.0 / b
    h = d
    for i in range(1, 10**7):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return h * _gamma_prefactor(a, x)


def chi2_tails(x, dof):
    """(lower, upper) tail probabilities of a chi-square with `dof` degrees of freedom at x, each computed directly where it is
    the small one (regularised incomplete gamma: series below the mean, continued fraction above)."""
    if dof <= 0:
        raise ValueError("dof must be positive")
    if x <= 0.0:
        return 0.0, 1.0
    if math.isinf(x):
        return 1.0, 0.0
    a, half = 0.5 * dof, 0.5 * x
    if half < a + 1.0:
        lower = min(1.0, _gamma_p_series(a, half))
        return lower, 1.0 - lower
    upper = min(1.0, _gamma_q_fraction(a, half))
    return 1.0 - upper, upper


def chi2_sf(x, dof):
    return chi2_tails(x, dof)[1]


def chi2_cdf(x, dof):
    return chi2_tails(x, dof)[0]


def z_to_p(z):
    """Two-sided tail probability of a standard normal deviate."""
    return math.erfc(abs(z) / math.sqrt(2.0))


# ---- statistics --------------------------------------------------------------------------------------------------------

MIN_EXPECTED = 10.0
MAX_REST_MASS = 0.01


def pooled_chi2(observed, expected_prob, num_samples):
    """Pearson's chi-square of a histogram of `num_samples` against exact bin probabilities.  Bins whose expected count is
    below 10 are merged into ONE rest bin that stays in the statistic (nothing is dropped); it may hold at most 1 % of the
    mass (asserted: choose rates and N accordingly).  A rest bin that itself expects fewer than 10 joins the smallest kept
    bin.  Returns (chi2, dof); dof = 0 when only one bin can occur (chi2 is then 0, or inf if an impossible bin is hit)."""
    observed = np.asarray(observed, dtype=np.float64).reshape(-1)
    prob = np.asarray(expected_prob, dtype=np.float64).reshape(-1)
    if observed.size != prob.size:
        raise ValueError("observed and expected_prob differ in size")
    if abs(float(observed.sum()) - num_samples) > 0.5:
        raise ValueError("the histogram does not hold num_samples")
    assert abs(float(prob.sum()) - 1.0) < 1e-9, prob.sum()
    expected = prob * float(num_samples)
    keep = expected >= MIN_EXPECTED
    rest_mass = float(prob[~keep].sum())
    assert rest_mass <= MAX_REST_MASS, "rest bin holds %.3g of the mass" % rest_mass
    obs, exp = observed[keep], expected[keep]
    rest_obs, rest_exp = float(observed[~keep].sum()), float(expected[~keep].sum())
    if rest_exp >= MIN_EXPECTED:
        obs, exp = np.append(obs, rest_obs), np.append(exp, rest_exp)
    elif rest_exp > 0.0 or rest_obs > 0.0:
        if rest_exp == 0.0:
            return float("inf"), max(0, obs.size - 1)
        low = int(np.argmin(exp))
        obs, exp = obs.copy(), exp.copy()
        obs[low] += rest_obs
        exp[low] += rest_exp
    return float(((obs - exp) ** 2 / exp).sum()), obs.size - 1


P_LIMIT = 1e-6


def chi2_verdict(chi2, dof):
    """(lower tail, upper tail, ok).  A case fails when either tail is below 10^-6: a histogram far from the distribution, or
    one implausibly close to it."""
    if dof == 0:
        return 1.0, 1.0, chi2 == 0.0
    lower, upper = chi2_tails(chi2, dof)
    return lower, upper, lower >= P_LIMIT and upper >= P_LIMIT


def z_verdict(observed, mean, var):
    """(z, two-sided p, ok) of a count against its exact mean and variance; var = 0 asks for equality."""
    if var <= 0.0:
        return 0.0, 1.0, float(observed) == float(mean)
    z = (float(observed) - mean) / math.sqrt(var)
    p = z_to_p(z)
    return z, p, p >= P_LIMIT


# ---- what both test files do with a statistic: print it once, then judge it ----------------------------------------------

def report(label, stat, dof, low, up):
    print("P-VALUE %-78s stat %14.6g dof %7d  lower %.3e  upper %.3e" % (label, stat, dof, low, up))


def assert_chi2_stat(label, chi2, dof):
    low, up, ok = chi2_verdict(chi2, dof)
    report(label, chi2, dof, low, up)
    assert ok, (label, chi2, dof, low, up)


def assert_chi2(label, observed, prob, count):
    assert_chi2_stat(label, *pooled_chi2(observed, prob, count))


def assert_z(label, observed, mean, var):
    z, p, ok = z_verdict(observed, mean, var)
    report(label + " (z)", z, 1, p, p)
    assert ok, (label, observed, mean, var, z, p)


def pair_table(a, b, bins):
    """Contingency counts of two integer sequences with values in [0, bins), flattened a-major."""
    return np.bincount(np.asarray(a, dtype=np.int64) * bins + np.asarray(b, dtype=np.int64), minlength=bins * bins)
