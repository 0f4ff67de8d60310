"""TEST INFRASTRUCTURE - the inputs of ``tests/test_moments_parity_gpu.py`` (``pf_moments`` / ``pf_forecast`` / ``pf_normalize`` /
``pf_loglik`` against the float64 oracle) as CPU generators, so that ``tests/test_moments_oracle_cpu.py`` can assert the INPUT
CONDITIONS of those comparisons - the oracle resolves every case; the raw one-pass formula does not - on exactly the inputs the
GPU tests use.  No product import.

Weighted clouds ``x (N, B, D)``, ``W (N, B)`` whose components sit at a LEVEL far from zero compared with their spread: what a
variance taken from raw second moments, ``S2 - 2 mu S1 + mu^2 S0``, loses to cancellation and ``sum W (x - mean)^2`` (the
reference, ``oracle.cpu_ref.get_filter_mean_and_variance``) does not.  Values are drawn in float32 and widened, so both dtypes
see the same numbers; a case whose numbers float32 cannot hold (ratio 1e8) is float64-only (``Case.dtypes``)."""
import functools
import math

import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
RATIOS = (0.0, 1e2, 1e4, 1e6)  # level / spread of a component; float64 also:
RATIO_F64_ONLY = 1e8
# tiles are 1 024 particles at these B (make_geom: vec = 4 iff N % 4 == 0): a single particle, less than a wave, one short of /
# exactly / one into the second tile, two whole tiles, 4 particles in the last of five tiles, 69 tiles and one particle
N_ALL = (1, 2, 7, 1023, 1024, 1025, 2048, 4100, 70001)
B_ALL = (1, 3)
D_ALL = (1, 2, 3, 4, 7)  # pf_moments: groups of PF_MAXD = 3 planes - 4 and 7 cross groups and end on a group of one plane
WEIGHTS = ("softmax", "cubed", "half_zero", "single_first", "single_last", "single_last_tile", "uniform", "sum_half")
SPREADS = (1.0, 0.01, 3.0)


def tile_elems(n, b, target=1024, block=256, max_tiles=1024):
    """``make_geom`` of ``csrc/pf_host.hpp``: the particles per tile of the tiled reductions."""
    vec = 4 if n % 4 == 0 else 1
    rounds_total = -(-n // (block * vec))
    r = max(min((rounds_total * b) // target, rounds_total), -(-rounds_total // max_tiles), 1 if vec == 4 else 4)
    return r * block * vec


def last_tile_start(n, b):
    t = tile_elems(n, b)
    return ((n - 1) // t) * t


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * ord(c) for i, c in enumerate("|".join(str(k) for k in key))) + 7919)


def _settle(w, target):
    """Float32-exact weights whose float64 sum is ``target`` to ~1e-13, not to float32's 1e-8: the rounding's residual goes onto the
    largest weight, what that leaves onto ever smaller ones (finer ulps).  Why: the reference's mean is ``sum W x``, off the
    centroid by ``(sum W - 1) * level``; at level / spread = 1e6 a residual of 1e-8 puts it 1e-2 spreads off, where its OWN
    variance moves by 2e-12 per rounding of the mean - more than the 1e-12 the oracle must resolve."""
    w = w.float().double()
    for col in range(w.shape[1]):
        for _ in range(6):
            r = target - float(w[:, col].sum())
            if r == 0.0:
                break
            ok = w[:, col] > 4.0 * abs(r)
            if not bool(ok.any()):
                break
            j = int(torch.where(ok, w[:, col], torch.full_like(w[:, col], math.inf)).argmin()) if _ else int(w[:, col].argmax())
            w[j, col] = float((w[j, col] + r).float())
    return w


def weights(kind, n, b, gen, exact32=True):
    """``(N, B)`` float64, exact in float32 with ``sum W`` settled (``_settle``); with ``exact32 = False`` plain float64.
    Normalised except ``sum_half`` (the reference does not divide by ``sum W``)."""
    if kind in ("softmax", "sum_half"):
        w = torch.softmax(torch.randn(n, b, generator=gen, dtype=F32).double(), 0)
        w = w * (0.5 if kind == "sum_half" else 1.0)
    elif kind in ("cubed", "half_zero"):
        w = torch.rand(n, b, generator=gen, dtype=F32).double().pow(3) + (1e-3 if n < 8 else 0.0)
        if kind == "half_zero" and n > 1:
            w[1::2] = 0.0
        w = w / w.sum(0)
    elif kind == "uniform":
        w = torch.full((n, b), 1.0 / n, dtype=F64)
    else:
        w = torch.zeros(n, b, dtype=F64)
        w[{"single_first": 0, "single_last": n - 1, "single_last_tile": last_tile_start(n, b)}[kind]] = 1.0
    return _settle(w, 0.5 if kind == "sum_half" else 1.0) if exact32 else w


def levels(ratio, b, d):
    """``(B, D)`` level / spread per column and component: ``ratio`` with alternating sign, or - ``"mixed"`` - every ratio in turn,
    starting with column 0 at 0 and column 1 at -1e6, so that a pivot from the wrong column or plane is far off."""
    if ratio == "mixed":
        seq = (0.0, -1e6, 1e4, -1e2, 1e6, 0.0, -1e4, 1e2)
        return torch.tensor([[seq[(3 * j + i) % len(seq)] for j in range(d)] for i in range(b)], dtype=F64) if d > 1 else \
            torch.tensor([[seq[i % len(seq)]] for i in range(b)], dtype=F64)
    return torch.tensor([[ratio * (-1.0) ** (i + j) for j in range(d)] for i in range(b)], dtype=F64)


class Case:
    def __init__(self, name, x, w, ratio, dtypes=("float64", "float32"), single=False, nan_at=None, equal=None):
        self.name, self.x, self.w, self.ratio, self.dtypes = name, x, w, ratio, dtypes
        self.single, self.nan_at, self.equal = single, nan_at, equal  # nan_at: (column, component); equal: the one value
        self.n, self.b, self.d = x.shape

    def __repr__(self):
        return self.name

    @property
    def finite(self):
        return self.nan_at is None

    def oracle(self):
        """``cpu_ref.get_filter_mean_and_variance`` in float64: ``(mean, var)``, each ``(B, D)``."""
        from oracle import cpu_ref

        return cpu_ref.get_filter_mean_and_variance(self.x, self.w, True)


def cloud(ratio, n, b, d, gen, exact32=True):
    lv = levels(ratio, b, d)
    sp = torch.tensor([SPREADS[j % len(SPREADS)] for j in range(d)], dtype=F64)
    x = (lv * sp + sp * torch.randn(n, b, d, generator=gen, dtype=F32).double())
    return x.float().double() if exact32 else x


def _case(ratio, n, b, d, wkind):
    f64_only = ratio == RATIO_F64_ONLY
    name = f"r{ratio if ratio == 'mixed' else format(ratio, '.0e')}-N{n}-B{b}-D{d}-{wkind}"
    gen = _gen(name)
    x = cloud(ratio, n, b, d, gen, exact32=not f64_only)
    # (ratio 1e8: sum W = 1 to float64's rounding - the reference's mean is sum W x, and (sum W - 1) * level must stay far below
    # the spread for its own variance to be resolved, tests/test_moments_oracle_cpu.py)
    w = weights(wkind, n, b, gen, exact32=not f64_only)
    return Case(name, x, w, float(levels(ratio, b, d).abs().max()), ("float64",) if f64_only else ("float64", "float32"),
                single=wkind.startswith("single"))


@functools.lru_cache(maxsize=None)
def cases():
    """The grid: every N at every ratio (B = 3, D = 4, the kinds of weights in turn); every D and B at the ratios that hurt; every
    kind of weights at three N; the degenerate clouds."""
    out, seen = [], set()

    def add(c):
        if c.name not in seen:
            seen.add(c.name)
            out.append(c)

    every_ratio = RATIOS + (RATIO_F64_ONLY, "mixed")
    for i, n in enumerate(N_ALL):
        for j, ratio in enumerate(every_ratio):
            add(_case(ratio, n, 3, 4, WEIGHTS[(i + j) % len(WEIGHTS)]))
    for i, d in enumerate(D_ALL):
        for b in B_ALL:
            for j, ratio in enumerate((1e6, "mixed", RATIO_F64_ONLY)):
                add(_case(ratio, 1025, b, d, ("softmax", "cubed", "half_zero", "sum_half")[(i + j + b) % 4]))
    for wkind in WEIGHTS:
        for n in (7, 1025, 4100):
            for ratio in (0.0, 1e4, 1e6):
                add(_case(ratio, n, 3, 2, wkind))
    # all particles equal to one large value
    for n, c, dts in ((1, 1e6, None), (1025, -3e6, None), (70001, 1e6 + 0.5, None), (4100, 123456789.125, ("float64",))):
        x = torch.full((n, 3, 2), c, dtype=F64)
        for wkind in ("cubed", "uniform"):
            add(Case(f"equal{c:g}-N{n}-{wkind}", x, weights(wkind, n, 3, _gen("equal", n, wkind)), math.inf,
                     dts or ("float64", "float32"), equal=c))
    # one NaN in component 2 of column 1 (the second group of planes), under a zero and under a positive weight
    for n, at in ((1025, 1024), (4100, 0), (4100, 2049)):
        for wkind in ("zero", "positive"):
            base = _case(1e6, n, 3, 4, "cubed")
            x, w = base.x.clone(), base.w.clone()
            x[at, 1, 2] = math.nan
            if wkind == "zero":
                w[at, 1] = 0.0
            assert wkind == "zero" or w[at, 1] > 0
            add(Case(f"nan@{at}-N{n}-w{wkind}", x, w, 1e6, nan_at=(1, 2)))
    return tuple(out)


def two_pass_longdouble(x, w):
    """``sum W x`` and ``sum W (x - mean)^2`` over axis 0 in numpy's extended precision."""
    xl, wl = x.numpy().astype(np.longdouble), w.numpy().astype(np.longdouble)[..., None]
    mean = (wl * xl).sum(0)
    return mean, (wl * (xl - mean) ** 2).sum(0)


def raw_one_pass(x, w):
    """The formula this grid exists to catch, in float64: ``S2 - 2 mu S1 + mu^2 S0`` from raw moments, clamped at 0."""
    ww = w.unsqueeze(-1)
    s0, s1, s2 = ww.sum(0), (ww * x).sum(0), (ww * x * x).sum(0)
    return s1, (s2 - 2.0 * s1 * s1 + s1 * s1 * s0).clamp_min(0.0)


def rel_err(got, ref):
    """``max |got - ref| / |ref|`` over the entries with ``ref != 0``; an entry with ``ref == 0`` must be met exactly (inf if not)."""
    got, ref = got.double().cpu(), ref.double()
    zero = ref == 0
    if bool((got[zero] != 0).any()):
        return math.inf
    return float(((got - ref).abs()[~zero] / ref.abs()[~zero]).max()) if bool((~zero).any()) else 0.0


# ---- pf_normalize / pf_loglik --------------------------------------------------------------------------------------------------
NORM_B = (1, 3, 300)
LOGW_KINDS = ("randn", "spread", "range", "single_finite", "all_neginf", "nonfinite", "side_by_side")


def logw(kind, n, b, dtype, salt=0):
    """Log-weights ``(N, B)`` in ``dtype``.  ``range``: more than 800 between the column's entries, the maximum in the last tile
    and everything else underflowing against it; ``side_by_side``: one column of each other kind next to each other."""
    gen = _gen("logw", kind, n, b, salt)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=F32).double()  # noqa: E731
    if kind == "side_by_side":
        kinds = [k for k in LOGW_KINDS if k != "side_by_side"]
        return torch.cat([logw(kinds[i % len(kinds)], n, 1, dtype, salt=i) for i in range(b)], 1)
    lw = rn(n, b)
    if kind == "spread":
        lw = 30.0 * lw - 700.0
    elif kind == "range":
        lw = lw - 900.0 * torch.rand(n, b, generator=gen, dtype=F32).double() - 50.0
        lw[last_tile_start(n, b) + (n - 1 - last_tile_start(n, b)) // 2] = 40.0
    elif kind == "single_finite":
        lw[:] = -math.inf
        lw[n // 2] = -3.0
    elif kind == "all_neginf":
        lw[:] = -math.inf
    elif kind == "nonfinite":
        # (always next to finite entries: among weights none of which is finite the kernels' equal shares are a documented
        # difference, INTEGRATION.md section 4b / tests/theta_oracle.py)
        for k, v in ((0, math.nan), (n - 1, math.inf), (n // 2, -math.inf), (n // 3, math.nan)):
            if n > 4 or (k == 0 and n > 1):
                lw[k] = v
    else:
        assert kind == "randn", kind
    return lw.to(dtype)


LOGLIK_KINDS = ("randn", "neginf_entries", "max_last_tile", "nan", "all_neginf")


def loglik_inputs(kind, n, b, dtype):
    """``v (N, B)`` and normalised ``W (N, B)`` with exact zeros (every third entry, never the whole column), in ``dtype``."""
    gen = _gen("loglik", kind, n, b)
    v = 3.0 * torch.randn(n, b, generator=gen, dtype=F32).double()
    if kind == "neginf_entries":
        v[::3] = -math.inf
        if n == 1:
            v[:] = -1.5
    elif kind == "max_last_tile":
        v = v - 200.0
        v[n - 1] = 25.0
    elif kind == "nan":
        v[n // 2, 0] = math.nan
    elif kind == "all_neginf":
        v[:, b - 1] = -math.inf
    else:
        assert kind == "randn", kind
    w = torch.rand(n, b, generator=gen, dtype=F32).double() + 1e-3
    if n > 2:
        w[1::3] = 0.0
        w[n - 1] = 0.5  # (the last particle - max_last_tile's maximum - keeps a weight: a float32 sum of the others alone underflows)
    w = (w / w.sum(0))
    return v.to(dtype), w.to(dtype)
