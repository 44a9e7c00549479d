"""NumPy twin of the counter-based dropout RNG in csrc/common.hpp (m3p_hash32 /
m3p_keep): the keep mask of every dropout site is a pure function of
(stream seed, linear element index), so tests can hand the oracle the exact mask a
kernel used and compare outputs / gradients element-wise with dropout switched on.  The same hash drives the seeded sampling
of the decoding loop (csrc/select.hip: m3p_vocab_sample); its twin - the uniforms, the keys and the whole draw in fp64 - is
at the end of this file."""
import numpy as np


def hash32(idx, seed):
    """m3p_hash32 of csrc/common.hpp (round 6: add the seed, three rounds of xor-shift-16 + 24-bit multiply-add, xor-shift-16)."""
    m32, m24, s16 = np.uint64(0xFFFFFFFF), np.uint64(0xFFFFFF), np.uint64(16)
    h = (np.asarray(idx, dtype=np.uint64) + np.uint64(int(seed) & 0xFFFFFFFF)) & m32
    for k in (0x9E3779, 0x85EBCB, 0xC2B2AF):
        h ^= h >> s16
        h = (h + (h & m24) * np.uint64(k)) & m32
    h ^= h >> s16
    return h.astype(np.uint32)


def keep_mask(n_elems, seed, p, shape=None):
    """Boolean keep mask for elements 0..n_elems-1 of a dropout stream: element i takes the low (i even) or high (i odd)
    16 bits of hash32(i >> 1) and is kept iff they are >= thresh24 >> 8, thresh24 = round(p * 2^24) (csrc/common.hpp:
    one hash serves two elements)."""
    thresh16 = int(round(float(p) * (1 << 24))) >> 8
    idx = np.arange(n_elems, dtype=np.uint64)
    h = hash32(idx >> np.uint64(1), seed)
    half = np.where((idx & np.uint64(1)) != 0, h >> np.uint32(16), h & np.uint32(0xFFFF))
    k = half >= np.uint32(thresh16)
    return k.reshape(shape) if shape is not None else k


def stream_seed(base_seed, step, site):
    """Per-(optimizer step, dropout site) 32-bit stream key; `site` enumerates the dropout
    call sites of the model (layer * 8 + k).  Plain integer mixing, identical on host and in tests."""
    x = (int(base_seed) * 0x9E3779B97F4A7C15 + int(step) * 0xBF58476D1CE4E5B9 + int(site) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    x ^= x >> 31
    x = (x * 0xD6E8FEB86659FD93) & (2 ** 64 - 1)
    x ^= x >> 32
    return int(x & 0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------------------
# Seeded sampling (csrc/select.hip: m3p_vocab_sample; decoder.generate(sample_seed=...)): the NumPy twin of the contract in
# include/m3p_hip.h, in fp64.  For row r and word w < V:  m = hash32(r * V + w, seed) >> 8,  u = (m + 0.5) 2^-24,
# E = -log(u),  key(r, w) = x[r, w] * inv_t - log(E);  the sampled word is the argmax of key over the allowed set, ties to the
# lowest word.  That is a draw from softmax(x * inv_t) on the allowed set but for the 24-bit grid of u: log(E) spans
# [-17.33, 2.85], so a word whose probability is below about 2^-24 of the most likely word's is never drawn.
# Nucleus (top-p) sampling (m3p_vocab_nucleus_sample; generate(sample_top_p=...)) cuts the allowed set to the words whose logit
# is >= nucleus_cut: the largest logit value at which the mass cumulated from the top reaches top_p - whole classes of equal
# logits.  top_p=None (and any value >= 1.0) is "off": every function below then returns what it returned without it.
# ---------------------------------------------------------------------------------------------------------------------
def inv_temperature(temperature):
    """1 / T as the fp32 number the kernel is handed (both routes of the decoder use this one value)."""
    t = float(temperature)
    if not t > 0.0:
        raise ValueError('the sampling temperature must be positive, got %r' % (temperature,))
    return float(np.float32(1.0 / t))


def sample_uniform(n, V, seed):
    """The exact u of every (row, word), fp64 [n, V] (every u is a 25-bit number: exact in fp64)."""
    assert int(n) * int(V) < 2 ** 32, 'the counter r * V + w is 32 bits'
    m = hash32(np.arange(int(n) * int(V), dtype=np.uint64), seed) >> np.uint32(8)
    return ((m.astype(np.float64) + 0.5) * 2.0 ** -24).reshape(int(n), int(V))


def sample_keys(x32, inv_t, seed):
    """The fp64 keys of fp32 logits x32 [n, V] (bf16 values on the device route); inv_t at its fp32 value."""
    x = np.asarray(x32, dtype=np.float32).astype(np.float64)
    assert x.ndim == 2
    u = sample_uniform(x.shape[0], x.shape[1], seed)
    return x * float(np.float32(inv_t)) - np.log(-np.log(u))


def nucleus_top_p(top_p):
    """top_p as the routes use it: None for "off" (None and any value >= 1.0), else its fp32 value in (0, 1) - what the
    kernel is handed.  Anything else (<= 0, NaN) raises ValueError."""
    if top_p is None:
        return None
    p = float(np.float32(top_p))
    if not p > 0.0:
        raise ValueError('top_p must satisfy 0 < top_p <= 1, got %r' % (top_p,))
    return None if p >= 1.0 else p


def nucleus_mass(x32, inv_t, cut, top_k=0):
    """Where a cut stands, in fp64, per row: (C(cut) / Z, C_above(cut) / Z) - the mass of the candidates (top_k as in
    sample_allowed) with a logit >= cut[r], and with a logit > cut[r], under softmax(x * inv_t) over the candidates."""
    x = np.asarray(x32, dtype=np.float32)
    cand = sample_allowed(x, top_k)
    y = np.where(cand, x.astype(np.float64) * float(np.float32(inv_t)), -np.inf)
    e = np.exp(y - y.max(axis=1)[:, None])                           # (a -inf logit and a word outside the candidates: mass 0)
    c = np.asarray(cut, dtype=np.float64).reshape(-1, 1)
    Z = e.sum(axis=1)
    return np.where(x >= c, e, 0.0).sum(axis=1) / Z, np.where(x > c, e, 0.0).sum(axis=1) / Z


def nucleus_cut(x32, inv_t, top_p, top_k=0):
    """The nucleus cut of every row, in fp64: (cut, C(cut) / Z, C_above(cut) / Z).  Over the candidate set K (top_k as in
    sample_allowed), with m = max_K x * inv_t:  mass(v) = #{w in K : x_w == v} * exp(v * inv_t - m) for each distinct logit
    value v,  C(v) = the sum of mass(v') over v' >= v,  C_above(v) the same over v' > v,  Z = C(-inf);  cut = max{v : C(v) >=
    top_p * Z}.  top_p at its fp32 value, like inv_t."""
    x = np.asarray(x32, dtype=np.float32)
    p = float(np.float32(top_p))
    assert 0.0 < p <= 1.0
    cand = sample_allowed(x, top_k)
    n, V = x.shape
    xs = -np.sort(-np.where(cand, x, -np.inf).astype(np.float64), axis=1)        # descending; outside K: -inf, mass 0
    e = np.exp(xs * float(np.float32(inv_t)) - xs[:, :1] * float(np.float32(inv_t)))
    e[np.isnan(e)] = 0.0                                                         # (-inf - -inf: a row without a finite logit)
    cs = np.cumsum(e, axis=1)
    col = np.arange(V)[None, :]
    last = np.ones((n, V), dtype=bool)
    last[:, :-1] = xs[:, :-1] != xs[:, 1:]                                       # the last entry of its class of equal logits
    last_at = np.minimum.accumulate(np.where(last, col, V)[:, ::-1], axis=1)[:, ::-1]
    C = np.take_along_axis(cs, last_at, axis=1)                                  # C(v) at every entry of v's class
    Z = cs[:, -1:]
    at = np.argmax(C >= p * Z, axis=1)[:, None]                                  # the first entry from the top that reaches it
    cut = np.take_along_axis(xs, at, axis=1)[:, 0]
    inside, above = nucleus_mass(x, inv_t, cut, top_k)
    return cut, inside, above


def sample_allowed(x32, top_k, top_p=None, inv_t=None):
    """Boolean [n, V]: top_k = 0 every word, else the row's first top_k words under (logit descending, word ascending).
    top_p (needs inv_t): of those, the words with a logit >= nucleus_cut - whole classes of equal logits, the smallest such
    set whose mass under softmax(x * inv_t) reaches top_p."""
    x = np.asarray(x32, dtype=np.float32)
    n, V = x.shape
    top_k = int(top_k)
    assert 0 <= top_k <= V
    if top_k == 0:
        allowed = np.ones((n, V), dtype=bool)
    else:
        order = np.argsort(-x, axis=1, kind='stable')[:, :top_k]     # stable: equal logits stay in word order
        allowed = np.zeros((n, V), dtype=bool)
        np.put_along_axis(allowed, order, True, axis=1)
    top_p = nucleus_top_p(top_p)
    if top_p is not None:
        assert inv_t is not None, 'the nucleus is a mass under softmax(x * inv_t)'
        allowed &= x >= nucleus_cut(x, inv_t, top_p, top_k)[0].astype(np.float32)[:, None]
    return allowed


def sample_words(x32, inv_t, seed, top_k=0, top_p=None):
    """The whole contract: (words int64 [n], logprob fp64 [n], key fp64 [n]) - the argmax of the keys over the allowed set
    (the lowest word among equal keys), logprob = x_w * inv_t - log-sum-exp of x * inv_t over the allowed set, and the
    winning key.  top_p: the allowed set is cut to the nucleus (sample_allowed)."""
    x = np.asarray(x32, dtype=np.float32)
    allowed = sample_allowed(x, top_k, top_p, inv_t)
    keys = np.where(allowed, sample_keys(x, inv_t, seed), -np.inf)
    words = np.argmax(keys, axis=1)                                  # (the first maximum: the lowest word)
    rows = np.arange(x.shape[0])
    assert allowed[rows, words].all(), 'a row without a finite logit in its allowed set'
    y = np.where(allowed, x.astype(np.float64) * float(np.float32(inv_t)), -np.inf)
    mx = y.max(axis=1)
    lse = mx + np.log(np.exp(y - mx[:, None]).sum(axis=1))
    return words.astype(np.int64), y[rows, words] - lse, keys[rows, words]
