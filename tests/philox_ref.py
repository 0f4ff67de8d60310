"""Host oracle of the in-kernel random numbers (TEST INFRASTRUCTURE; numpy, no GPU).

A restatement of what ``pyfilter_amd/csrc/pf_philox.hpp`` promises, written from the Philox paper (Salmon, Moraes, Dror, Shaw:
"Parallel random numbers: as easy as 1, 2, 3", SC'11 - the 4x32 bijection with ten rounds, the two multipliers and the two Weyl
key increments of its table 2) and from the header's comments on addressing:

* one call = four 32-bit words, counter = (element low word, element high word, step, stream), key = (seed low, seed high);
* a word becomes a number by its top 24 bits (float32) or by the top 53 bits of two consecutive words (float64), closed at 0
  (``u01``) or open at 0 (``u01_open0``: never 0, so a logarithm is safe);
* standard normals are Box-Muller pairs addressed by the flat number ``n = element * D + d``: four per call in float32 (words
  (x, y) then (z, w)), two per call in float64 (one pair from the two 53-bit uniforms);
* Exp(1) spacings of the multinomial resampler live on the multinomial stream with ``0x200`` ORed into the stream word, one per
  word (float32) or per word pair (float64), the element being the call-and-word number;
* a uniform draw takes the first word (float32) or the first two (float64) of the call addressed by the element itself.

Everything is evaluated in float64 whatever ``dtype`` says: ``dtype`` selects the ADDRESSING and the number of random bits, the
kernels' float32 transcendentals are somebody else's business (the tests compare within bars that a wrong word overshoots by
orders of magnitude).

The jitter kernel's draws are restated on top of this module by ``tests/theta_oracle.py::jitter_draws``."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
# table 2 of the paper, philox4x32
_MUL_A, _MUL_B = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_WEYL_A, _WEYL_B = 0x9E3779B9, 0xBB67AE85  # golden ratio, sqrt(3) - 1
ROUNDS = 10

# the stream words of the library (tests/test_philox_cpu.py checks them against the sources)
STREAMS = dict(NORMAL=0, UNIFORM=1, INIT=2, MULTINOMIAL=3, SMOOTH=5, NESTED_Z=6, NESTED_PICK=7, FORECAST_Z=8, FORECAST_E=9,
               SMOOTH_MH=10, JITTER=0x4A495454)
EXP_FLAG = 0x200  # ORed into the stream word of the Exp(1) spacings


def _u64(v):
    return np.asarray(v, dtype=np.uint64)


def _round(ctr, key):
    """One S-P round of the paper's figure 1 on the four counter words."""
    a, b, c, d = ctr
    prod_a, prod_c = _MUL_A * a, _MUL_B * c  # 32 x 32 -> 64 bits: exact in uint64
    return ((prod_c >> np.uint64(32)) ^ b ^ key[0], prod_c & M32, (prod_a >> np.uint64(32)) ^ d ^ key[1], prod_a & M32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on ``uint64`` arrays holding 32-bit words (broadcast against each other): the four output words."""
    ctr = tuple(np.broadcast_arrays(*[_u64(c) & M32 for c in (c0, c1, c2, c3)]))
    k0, k1 = _u64(k0) & M32, _u64(k1) & M32
    schedule = [((k0 + np.uint64((r * _WEYL_A) & 0xFFFFFFFF)) & M32, (k1 + np.uint64((r * _WEYL_B) & 0xFFFFFFFF)) & M32)
                for r in range(ROUNDS)]
    for key in schedule:
        ctr = _round(ctr, key)
    return ctr


def call(seed, stream, step, counter):
    """The four words of call number ``counter`` (array) of (seed, stream, step)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    counter = _u64(counter)
    return philox4x32_10(counter & M32, counter >> np.uint64(32), np.uint64(int(step) & 0xFFFFFFFF), np.uint64(int(stream)),
                         np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))


# ---- word -> number -------------------------------------------------------------------------------------------------------
def u01(a):
    return (_u64(a) >> np.uint64(8)).astype(np.float64) / 2.0 ** 24


def u01_open0(a):
    return ((_u64(a) >> np.uint64(8)).astype(np.float64) + 1.0) / 2.0 ** 24


def _bits53(a, b):
    return (((_u64(a) << np.uint64(32)) | _u64(b)) >> np.uint64(11)).astype(np.float64)  # < 2^53: exact


def u01_d(a, b):
    return _bits53(a, b) / 2.0 ** 53


def u01_open0_d(a, b):
    return (_bits53(a, b) + 1.0) / 2.0 ** 53


def _is32(dtype):
    name = str(dtype)
    if name.endswith("float32"):
        return True
    assert name.endswith("float64"), dtype
    return False


def _pick(words, which):
    out = np.zeros(which.shape, dtype=np.float64)
    for k, w in enumerate(words):
        out = np.where(which == k, w, out)
    return out


# ---- address maps: (call number, slot inside the call) of a draw - THE maps of this module; the draws below go through them, and
# tests/test_philox_cpu.py shows them injective --------------------------------------------------------------------------------
def slots_per_call(dtype):
    """Numbers one call yields: four (one per word) in float32, two (one per word pair) in float64."""
    return 4 if _is32(dtype) else 2


def slot_words(slot, dtype):
    """The 32-bit words of a call that slot ``slot`` owns: word ``slot`` (float32) or the pair ``2 slot, 2 slot + 1`` (float64).
    (The two normals of a Box-Muller pair are functions of ALL the words of their pair - float32: slots 0, 1 of words x, y and slots
    2, 3 of z, w; float64: slots 0, 1 of all four: each is counted as owning its share of them.)"""
    return (int(slot),) if _is32(dtype) else (2 * int(slot), 2 * int(slot) + 1)


def normal_address(elem, D, dtype):
    """Normal ``d`` of element ``elem`` is number ``n = elem D + d`` of its (stream, step): ``(call, slot)`` arrays ``elem.shape + (D,)``."""
    n = _u64(elem)[..., None] * np.uint64(D) + np.arange(D, dtype=np.uint64)
    per = np.uint64(slots_per_call(dtype))
    return n // per, n % per


def exponential_address(elem, dtype):
    """Spacing ``elem``: call ``elem >> 2`` / slot ``elem & 3`` (float32), call ``elem >> 1`` / slot ``elem & 1`` (float64)."""
    elem = _u64(elem)
    shift = np.uint64(2 if _is32(dtype) else 1)
    return elem >> shift, elem & ((np.uint64(1) << shift) - np.uint64(1))


def uniform_address(elem, dtype):
    """A uniform draw has a call of its own - number ``elem`` - and takes slot 0."""
    elem = _u64(elem)
    return elem, np.zeros_like(elem)


def _slot_values(r, dtype, one, two):
    """The number every slot of the calls ``r`` (four word arrays) yields: ``one(word)`` / ``two(high word, low word)``."""
    return [one(r[slot_words(k, dtype)[0]]) if _is32(dtype) else two(*[r[w] for w in slot_words(k, dtype)])
            for k in range(slots_per_call(dtype))]


# ---- the draws ------------------------------------------------------------------------------------------------------------
def normals(seed, stream, step, elem, D, dtype, words=(0, 1, 2, 3)):
    """Standard normals ``elem.shape + (D,)`` of the elements ``elem`` (float64 values).  ``words``: which of the call's four
    words plays x, y, z, w - the identity; the mutation checks of the tests pass another order."""
    at, slot = normal_address(elem, D, dtype)
    r = call(seed, stream, step, at)
    if _is32(dtype):
        x, y, z, w = (r[k] for k in words)
        rad_a, rad_b = np.sqrt(-2.0 * np.log(u01_open0(x))), np.sqrt(-2.0 * np.log(u01_open0(z)))
        ang_a, ang_b = 2.0 * np.pi * u01(y), 2.0 * np.pi * u01(w)
        return _pick((rad_a * np.cos(ang_a), rad_a * np.sin(ang_a), rad_b * np.cos(ang_b), rad_b * np.sin(ang_b)), slot)
    x, y, z, w = r
    rad, ang = np.sqrt(-2.0 * np.log(u01_open0_d(x, y))), 2.0 * np.pi * u01_d(z, w)
    return _pick((rad * np.cos(ang), rad * np.sin(ang)), slot)


def exponentials(seed, step, elem, dtype):
    """Exp(1) spacings of the elements ``elem`` (multinomial stream | 0x200)."""
    at, slot = exponential_address(elem, dtype)
    r = call(seed, STREAMS["MULTINOMIAL"] | EXP_FLAG, step, at)
    return -np.log(_pick(_slot_values(r, dtype, u01_open0, u01_open0_d), slot))


def uniform(seed, stream, step, elem, dtype):
    """The uniform in [0, 1) of element ``elem``: exact in ``dtype`` (24 / 53 bits)."""
    at, slot = uniform_address(elem, dtype)
    return _pick(_slot_values(call(seed, stream, step, at), dtype, u01, u01_d), slot)


def positions_from_spacings(e, tail, dtype):
    """Order statistics of ``len(e)`` uniforms from Exp(1) spacings: ``cumsum(e) / (sum(e) + tail)``; (float64, rounded to dtype)."""
    p = np.cumsum(np.asarray(e, dtype=np.float64)) / (np.sum(e, dtype=np.float64) + float(tail))
    return p, (p.astype(np.float32).astype(np.float64) if _is32(dtype) else p)


def multinomial_positions(seed, step, b, N, B, dtype):
    """The sorted resampling positions of filter ``b`` of ``B`` filters of ``N`` particles at ``step``: spacings of the elements
    ``b N .. b N + N - 1``, the tail spacing (the gap above the largest position) at element ``B N + b``."""
    e = exponentials(seed, step, b * N + np.arange(N, dtype=np.uint64), dtype)
    tail = exponentials(seed, step, np.array([B * N + b], dtype=np.uint64), dtype)[0]
    return positions_from_spacings(e, tail, dtype)


# ---- ancestors ------------------------------------------------------------------------------------------------------------
def cdf64(W):
    """float64 cumulative sum of normalised weights ``(N,)`` with its last entry pinned to 1 (what the resamplers search)."""
    c = np.cumsum(np.asarray(W, dtype=np.float64))
    c[-1] = 1.0
    return c


def valid_ancestor(a, p, cdf, delta):
    """Is ``a`` the left-side searchsorted of SOME position within ``delta`` of ``p``?  ``cdf[a] >= p - delta`` and (``a == 0`` or
    ``cdf[a - 1] < p + delta``).  An ancestor that differs from the exact one therefore implies a cdf entry within ``delta`` of
    ``p``; an index clamped to ``N - 1`` is valid there because the last entry is 1."""
    a = np.asarray(a, dtype=np.int64)
    p = np.asarray(p, dtype=np.float64)
    inside = (a >= 0) & (a < len(cdf))
    ac = np.clip(a, 0, len(cdf) - 1)
    below = np.where(ac > 0, cdf[np.maximum(ac - 1, 0)], -np.inf)
    return inside & (cdf[ac] >= p - delta) & (below < p + delta)


def near_boundary(p, cdf, delta):
    """Which positions lie within ``delta`` of a cdf entry (where the slack of ``valid_ancestor`` can matter at all)."""
    p = np.asarray(p, dtype=np.float64)
    j = np.clip(np.searchsorted(cdf, p), 0, len(cdf) - 1)
    gap = np.minimum(np.abs(cdf[j] - p), np.abs(cdf[np.maximum(j - 1, 0)] - p))
    return gap <= delta
