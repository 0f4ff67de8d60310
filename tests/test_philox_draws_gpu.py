"""Every mode in which a kernel draws its OWN random numbers, pinned to the host oracle of the generator (``tests/philox_ref.py``;
its known answers and address maps: ``tests/test_philox_cpu.py``).

The exact comparisons of the rest of the suite run on taped draws; the generator's own modes were held to moments and chi-squares,
which an addressing collision - two particles, filters, components or streams reading one 32-bit word - passes.  Here:

a. ``pf_debug_draw_normals`` (the record of what a fused run drew) against ``normals()``;
b. the fused multinomial resampler (step kernel MODE 1, column kernel): the ancestors of a teacher-forced move against the oracle's
   order statistics and the float64 cdf of the teacher's weights (``valid_ancestor``: left-side searchsorted for some position within
   ``delta``), the new particles against ``oracle.models.propagate`` on the oracle's normals;
c. the stand-alone ``pf_multinomial(v = NULL)`` against searchsorted at the oracle's uniforms;
d. the Philox systematic offset (``filter_block``: the kernels draw it) against ``cpu_ref.systematic`` fed the oracle's uniform;
e. own-draw mode = taped mode fed the regenerated draws, for ``pf_sample_and_weight``, ``pf_initial_sample[_cols]``,
   ``pf_nested_sample_and_weight``, ``pf_forecast`` and ``pf_smooth_ffbs``.

A fused run numbers its moves from 0 and keys its draws by that number, whatever the time index of the state it starts from: a
one-move run has step word 0, the second move of a two-move run step word 1 - and consumes the spacing sums its predecessor left in
the partials.  The runs' Philox seed is pinned through the replay token (``tests/philox_cases.py: RUN_SEED``).

Bars (``tests/philox_cases.py``): positions ``delta`` 1e-12 (float64) / 2e-6 (float32); float64 values 1e-12 relative; float32 normals
1e-3 absolute against the float64 evaluation on the same bits - a bar about addressing (a wrong word moves a normal by O(1), thousands
are compared), not about the hardware transcendentals.  Every model used here moves a particle by at most 1 per unit of its normal,
so ``1e-3`` on the normals is ``1e-3`` on the float32 particles of the own-draw / taped comparisons.

Each assertion is shown to bite by a MUTATION OF THE HOST RESTATEMENT, run next to it (never a broken kernel): see ``_mutations_bite``
and ``test_generator``.  The figures the tests print (``philox-parity:`` lines) are recorded in ``profiles/philox_parity.txt``.

The jitter and theta kernels keep their draws for a later change."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from oracle import models as M
from oracle.cases import build_spec
from pyfilter_amd import _lib as L
from pyfilter_amd import ops
from tests import philox_cases as PC
from tests import philox_ref as P
from tests.helpers import build_ssm_from_case
from tests.nested_cases import rounded_spec

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DTYPES = [F32, F64]
S = P.STREAMS


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A device error is sticky: nothing of this module runs on the device after one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, the remaining cases are not run: {e}", returncode=3)


def _name(dtype):
    return "float32" if dtype == F32 else "float64"


def _say(*a):
    print("philox-parity:", *a)


def _value_bar(dtype, ref):
    """|got - ref| allowed for a VALUE that is one normal times a scale <= 1 plus a location ``ref``."""
    return PC.VALUE_F64 * (1.0 + ref.abs()) if dtype == F64 else torch.full_like(ref, PC.NORMAL_F32)


def _weight_error(own_w, tap_w):
    """float64 log-weights, own draws against taped: the largest ``|dw| / (1 + |w|)`` over the finite ones (the same ones)."""
    own_w, tap_w = own_w.double().cpu(), tap_w.double().cpu()
    fin = torch.isfinite(tap_w)
    assert torch.equal(fin, torch.isfinite(own_w)) and torch.equal(own_w[~fin].isnan(), tap_w[~fin].isnan())
    return float(((own_w[fin] - tap_w[fin]).abs() / (1.0 + tap_w[fin].abs())).max()) if bool(fin.any()) else 0.0


# ---- a. the generator ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [PC.SEED_LOW, PC.SEED_HIGH], ids=["seed_both_halves", "seed_above_2_63"])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_generator(dtype, d, seed):
    worst = 0.0
    for n, b in ((5, 1), (333, 3), (1024, 2), (4100, 2)):
        for step0 in (0, 7):
            got = ops.debug_draw_normals(seed, 2, n, b, d, dtype, "cuda", step0=step0).cpu().double()  # (steps, D, B, N)
            for s in range(2):
                ref = PC.oracle_normals(seed, S["NORMAL"], step0 + s, n, b, d, _name(dtype)).permute(2, 1, 0)  # (D, B, N)
                err = (got[s] - ref).abs()
                bar = PC.NORMAL_F32 if dtype == F32 else PC.VALUE_F64 * (1.0 + ref.abs())
                worst = max(worst, float(err.max()))
                assert bool((err <= bar).all()), f"{n}x{b} D={d} step {step0 + s}: {int((err > bar).sum())} normals off, worst {float(err.max()):.3e}"
                if dtype == F32 and n >= 333:
                    # MUTATION: words y and z of a float32 call swapped in the restatement -> the comparison must fail
                    swapped = PC.oracle_normals(seed, S["NORMAL"], step0 + s, n, b, d, "float32", words=(0, 2, 1, 3)).permute(2, 1, 0)
                    assert float(((got[s] - swapped).abs() > PC.NORMAL_F32).double().mean()) > 0.5
    _say(f"generator {_name(dtype)} D={d} seed={seed:#x}: largest |normal - oracle| {worst:.3e}")


# ---- b. the fused multinomial resampler ------------------------------------------------------------------------------------------
def _filter(case, dtype, resampler):
    from pyfilter_amd import resampling
    from pyfilter_amd.filters.particle import APF, SISR, proposals

    ssm = build_ssm_from_case(case, dtype, "cuda")
    cls = {"sisr": SISR, "apf": APF}[case["filter"]]
    prop = {"bootstrap": proposals.Bootstrap, "lgo": proposals.LinearGaussianObservations}[case["proposal"]]()
    filt = cls(ssm, case["N"], proposal=prop, resampling=getattr(resampling, resampler), ess_threshold=case["ess_threshold"], seed=5)
    filt.set_batch_shape(torch.Size([case["B"]]))
    return filt


def _teacher_state(filt, t, x, logw):
    from pyfilter_amd.filters.particle.state import ParticleFilterCorrection
    from pyfilter_amd.timeseries import TimeseriesState

    n, b = logw.shape
    idx = torch.arange(n).unsqueeze(-1).expand(n, b).contiguous()
    return ParticleFilterCorrection(TimeseriesState(t, x.cuda(), filt._model.hidden.event_shape), logw.clone().cuda(),
                                    torch.zeros(b, dtype=logw.dtype, device="cuda"), idx.cuda())


def _route(monkeypatch, route, tile_target=0):
    from pyfilter_amd.hints import HINTS

    monkeypatch.setattr(HINTS, "route", {"column": 0, "step": 1, "cluster": 4}[route])
    monkeypatch.setattr(HINTS, "tile_target", tile_target)


def _block(filt, y, state, moves, route, mode, multi=None):
    """``moves`` moves from ``state`` as one fused run keyed with ``RUN_SEED``; the launch trace must show the route under test."""
    res, ll_steps, _ = filt.filter_block(y[:moves].cuda(), state, replay=(PC.RUN_SEED, None))
    torch.cuda.synchronize()
    trace = ops.debug_launch_trace(moves)
    if route == "column":
        assert trace[-1]["SPEC"] == 9, trace
    elif route == "cluster":
        assert trace[-1]["SPEC"] == 10, trace
    else:
        assert [r["step"] for r in trace] == list(range(moves)) and all(r["SPEC"] not in (9, 10) and r["MODE"] == mode for r in trace), trace
        if multi is not None:
            assert all(r["MULTI"] == multi for r in trace), trace
    assert filt._last_run["seed_eff"] == PC.RUN_SEED
    last = res.latest_state
    return last.timeseries_state.value.cpu(), last.weights.cpu(), last.previous_indices.cpu(), ll_steps.cpu()


def _mutations_bite(anc, step, W, dtype, delta, seed=PC.RUN_SEED):
    """The ancestor check on MUTATED restatements must fail (each mutation still yields sorted, in-range, uniform positions):
    the tail spacing dropped from the total; the spacings of step + 1; filter b addressed at b (N + 1)."""
    n, b = W.shape
    name = _name(dtype)

    def no_tail(seed, st, k, n_, b_, dt):
        return P.positions_from_spacings(P.exponentials(seed, st, k * n_ + np.arange(n_, dtype=np.uint64), dt), 0.0, dt)

    def next_step(seed, st, k, n_, b_, dt):
        return P.multinomial_positions(seed, st + 1, k, n_, b_, dt)

    def one_off(seed, st, k, n_, b_, dt):
        e = P.exponentials(seed, st, k * (n_ + 1) + np.arange(n_, dtype=np.uint64), dt)
        return P.positions_from_spacings(e, P.exponentials(seed, st, np.array([b_ * n_ + k], dtype=np.uint64), dt)[0], dt)

    counts = []
    for label, fn in (("tail dropped", no_tail), ("step + 1", next_step), ("filter at b (N + 1)", one_off)):
        invalid, _ = PC.check_ancestors(anc, seed, step, W, name, delta, positions=fn)
        counts.append(f"{label}: {invalid}")
        # (a dropped tail moves position p by p tail / sum, ~ Exp(1) / N at most: it shows in a few per cent of the ancestors;
        # the other two redraw every position)
        assert invalid > (0 if fn is no_tail else 0.02 * n), f"the mutation '{label}' passes the ancestor check ({invalid} of {n * b} invalid)"
    return "invalid under the mutations - " + ", ".join(counts)


def _check_sisr_move(tag, case, dtype, x_in, w_in, step, x_out, anc, seed=PC.RUN_SEED):
    """One multinomial SISR + Bootstrap move of the kernels from ``(x_in, w_in)`` at step word ``step``: returns the slack count."""
    name, delta = _name(dtype), PC.DELTA[dtype]
    n, b = w_in.shape
    W = PC.weights64(w_in)
    shares = PC.near_share(seed, step, W, name, delta)
    assert max(shares) <= PC.NEAR_SHARE, f"{tag}: input condition - {shares} of the positions lie within {delta:g} of a cdf entry"
    assert bool((anc[1:] >= anc[:-1]).all()), f"{tag}: ancestors decrease"
    invalid, slack = PC.check_ancestors(anc.numpy(), seed, step, W, name, delta)
    _say(f"{tag} {name} step word {step}: {invalid} invalid, {slack} of {n * b} ancestors needed the slack; share of positions within "
         f"{delta:g} of a cdf entry (host) {max(shares):.4f}")
    assert invalid == 0, f"{tag}: {invalid} ancestors are no searchsorted of the oracle's positions within {delta:g}"
    if dtype == F64:
        assert slack == 0, f"{tag}: {slack} float64 ancestors differ from the exact search"
    if n >= 333:
        _say(f"{tag} {name} step word {step}:", _mutations_bite(anc.numpy(), step, W, dtype, delta, seed))
    # the new particles: the transition from the ancestors the kernel named, on the oracle's normals
    spec = rounded_spec(case, dtype)
    d = max(1, spec.dim)
    z = PC.oracle_normals(seed, S["NORMAL"], step, n, b, d, name)
    ref = M.propagate(spec, cpu_ref.batched_gather(x_in.double(), anc, 0), z if spec.dim > 0 else z[..., 0])
    err = (x_out.double() - ref).abs()
    scale = float(ref.abs().max())
    bar = PC.VALUE_F64 * scale if dtype == F64 else 1e-5 * scale + 1e-6
    _say(f"{tag} {name} step word {step}: largest |x - oracle| {float(err.max()):.3e} (bar {bar:.3e})")
    assert bool((err <= bar).all()), f"{tag}: {int((err > bar).sum())} particles off, worst {float(err.max()):.3e} (bar {bar:.3e})"
    return slack


def _sisr_two_moves(monkeypatch, route, model, n, b, dtype, tile_target=0, multi=None):
    _route(monkeypatch, route, tile_target)
    case = PC.case_of(model, "sisr", "bootstrap", n, b)
    y = PC.observations(case, dtype)
    filt = _filter(case, dtype, "multinomial")
    x0, w0 = PC.teacher(case, dtype)
    tag = f"{route} {model} {n}x{b}"
    # one move from the teacher state (time index 3) ...
    x1, w1, anc1, ll1 = _block(filt, y, _teacher_state(filt, 3, x0, w0), 1, route, 1, multi)
    _check_sisr_move(tag + " move 1", case, dtype, x0, w0, 0, x1, anc1)
    # ... and the same run one move longer: its second move starts from the state just checked (the same draws: a cut replay)
    x2, _, anc2, ll2 = _block(filt, y, _teacher_state(filt, 3, x0, w0), 2, route, 1, multi)
    assert torch.equal(ll2[0], ll1[0]), "the first move of the longer run is not the one-move run"
    _check_sisr_move(tag + " move 2", case, dtype, x1, w1, 1, x2, anc2)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n,b", PC.COLUMN_SHAPES)
@pytest.mark.parametrize("model", PC.MODELS)
def test_fused_multinomial_column_kernel(model, n, b, dtype, monkeypatch):
    _sisr_two_moves(monkeypatch, "column", model, n, b, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n,b,tile_target", PC.STEP_SHAPES)
@pytest.mark.parametrize("model", PC.MODELS)
def test_fused_multinomial_step_kernel(model, n, b, tile_target, dtype, monkeypatch):
    multi = 1 if (tile_target or n % 4) else 0  # (tiles of several rounds: the MULTI instantiations)
    _sisr_two_moves(monkeypatch, "step", model, n, b, dtype, tile_target, multi)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("route,model,n,b", [("column", "sine", 333, 3), ("step", "lorenz", 4100, 2)])
def test_fused_multinomial_through_batch_filter(route, model, n, b, dtype, monkeypatch):
    """The same move issued by ``batch_filter(..., init_state=...)`` - the driver of a plain run - under the seed the filter gives the
    run itself (``_last_run["seed_eff"]``: its own seed plus the run's epoch), not a replay token."""
    _route(monkeypatch, route)
    case = PC.case_of(model, "sisr", "bootstrap", n, b)
    filt = _filter(case, dtype, "multinomial")
    x0, w0 = PC.teacher(case, dtype)
    res = filt.batch_filter(PC.observations(case, dtype)[:1].cuda(), bar=False, init_state=_teacher_state(filt, 3, x0, w0))
    torch.cuda.synchronize()
    rec = ops.debug_launch_trace(1)[-1]
    assert (rec["SPEC"] == 9) if route == "column" else (rec["SPEC"] not in (9, 10) and rec["MODE"] == 1), rec
    seed = filt._last_run["seed_eff"]
    assert seed not in (PC.RUN_SEED, 5)
    last = res.latest_state
    _check_sisr_move(f"batch_filter {route} {model} {n}x{b}", case, dtype, x0, w0, 0, last.timeseries_state.value.cpu(),
                     last.previous_indices.cpu(), seed)


@pytest.mark.parametrize("route,n,b", [("column", 333, 3), ("column", 1502, 3), ("step", 333, 3), ("step", 4100, 2)])
@pytest.mark.parametrize("model", ["sine", "rw2d"])
def test_fused_multinomial_apf_optimal_proposal_float64(model, route, n, b, monkeypatch):
    """APF + LinearGaussianObservations, float64: the cdf is that of the FIRST-STAGE weights ``pre_weight + log w`` - the oracle is
    taught ``cpu_ref``'s (``apf_step``), ``delta = 1e-11``."""
    _route(monkeypatch, route)
    case = PC.case_of(model, "apf", "lgo", n, b)
    spec = build_spec(case, F64)
    y = PC.observations(case, F64)
    filt = _filter(case, F64, "multinomial")
    x0, w0 = PC.teacher(case, F64)
    _, _, anc, _ = _block(filt, y, _teacher_state(filt, 3, x0, w0), 1, route, 1)
    W = PC.weights64(cpu_ref.lgo_pre_weight(spec, y[0], x0) + w0)
    shares = PC.near_share(PC.RUN_SEED, 0, W, "float64", PC.DELTA_APF)
    assert max(shares) <= PC.NEAR_SHARE
    assert bool((anc[1:] >= anc[:-1]).all())
    invalid, slack = PC.check_ancestors(anc.numpy(), PC.RUN_SEED, 0, W, "float64", PC.DELTA_APF)
    _say(f"{route} apf+lgo {model} {n}x{b} float64: {invalid} invalid, {slack} of {n * b} ancestors needed the slack; share of positions "
         f"within {PC.DELTA_APF:g} of a cdf entry (host) {max(shares):.4f}")
    assert invalid == 0 and slack == 0
    _say(f"{route} apf+lgo {model} {n}x{b} float64:", _mutations_bite(anc.numpy(), 0, W, F64, PC.DELTA_APF))


# ---- c. the stand-alone multinomial resampler --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n,b", PC.MULTINOMIAL_SHAPES)
def test_stand_alone_multinomial(n, b, dtype):
    """Element ``e = b N + i`` draws ``uniform(seed, MULTINOMIAL, step, e)`` - exact in either type - and takes its left-side
    searchsorted in the cdf: only the cdf's ``delta`` applies.  The taped call on the regenerated uniforms gives the same indices."""
    name, delta, seed, step = _name(dtype), PC.DELTA[dtype], PC.SEED_LOW, 5
    W = PC.weights64(PC.teacher_logw(n, b, dtype)).to(dtype)  # (N, B) normalised, as the kernel is handed them
    Wc = ops.to_cols(W.cuda())
    idx = ops.multinomial_cols(Wc, seed, step).cpu().long()  # (B, N)
    u = np.stack([P.uniform(seed, S["MULTINOMIAL"], step, k * n + np.arange(n, dtype=np.uint64), name) for k in range(b)])
    taped = ops.multinomial_cols(Wc, seed + 1, step + 1, v=torch.from_numpy(u).to(dtype).cuda()).cpu().long()
    assert torch.equal(idx, taped), f"{int((idx != taped).sum())} indices differ from the taped call on the regenerated uniforms"
    slack, shares = 0, []
    for k in range(b):
        cdf = P.cdf64(W[:, k].double().numpy() / float(W[:, k].double().sum()))
        shares.append(float(P.near_boundary(u[k], cdf, delta).mean()))
        ok = P.valid_ancestor(idx[k].numpy(), u[k], cdf, delta)
        assert ok.all(), f"filter {k}: {int((~ok).sum())} indices are no searchsorted of the oracle's uniform"
        slack += int((idx[k].numpy() != np.minimum(np.searchsorted(cdf, u[k]), n - 1)).sum())
        # MUTATION: the uniforms of the next filter's elements (an offset one column off) must fail
        other = P.uniform(seed, S["MULTINOMIAL"], step, (k + 1) * n + np.arange(n, dtype=np.uint64), name)
        assert n < 333 or not P.valid_ancestor(idx[k].numpy(), other, cdf, delta).all()
    _say(f"pf_multinomial {n}x{b} {name}: {slack} of {n * b} indices needed the slack; share of uniforms within {delta:g} of a cdf entry "
         f"(host) {max(shares):.4f}")
    assert max(shares) <= PC.NEAR_SHARE
    if dtype == F64:
        assert slack == 0


# ---- d. the Philox systematic offset -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("route,n,b", [("step", 4100, 2), ("column", 333, 3), ("cluster",) + PC.CLUSTER_SHAPE])
@pytest.mark.parametrize("filt_name,prop", [("sisr", "bootstrap"), ("apf", "lgo")])
def test_philox_systematic_offset(filt_name, prop, route, n, b, dtype, monkeypatch):
    """No ``u`` tape: the kernels draw the move's offset ``uniform(seed, UNIFORM, step, b)``.  The ancestors are those of
    ``cpu_ref``'s systematic resampler fed that number: identical in float64, through ``valid_ancestor`` in float32 - for the first
    move of a run (step word 0) and for the second (step word 1), teacher-forced from the state the first ended in."""
    _route(monkeypatch, route)
    name, delta = _name(dtype), PC.DELTA[dtype]
    case = PC.case_of("sine", filt_name, prop, n, b)
    spec = rounded_spec(case, dtype)
    y = PC.observations(case, dtype)
    filt = _filter(case, dtype, "systematic")
    x0, w0 = PC.teacher(case, dtype)

    def check(move, x_in, w_in, anc):
        """The ancestors of move ``move`` (step word ``move - 1``) from ``(x_in, w_in)``."""
        step = move - 1
        rw = w_in.double() if filt_name == "sisr" else cpu_ref.lgo_pre_weight(spec, y[step].double(), x_in.double()) + w_in.double()
        W = PC.weights64(rw)
        u = P.uniform(PC.RUN_SEED, S["UNIFORM"], step, np.arange(b, dtype=np.uint64), name)
        ref = cpu_ref.systematic(W, normalized=True, u=torch.from_numpy(u).reshape(b, 1))
        differ = int((anc != ref).sum())
        grids = [(np.arange(n) + u[k]) / n for k in range(b)]
        share = max(float(P.near_boundary(grids[k], P.cdf64(W[:, k].numpy()), delta).mean()) for k in range(b))
        _say(f"systematic offset {route} {filt_name}+{prop} {n}x{b} {name} step word {step}: {differ} of {n * b} ancestors differ from "
             f"cpu_ref's; share of grid positions within {delta:g} of a cdf entry (host) {share:.4f}")
        assert share <= PC.NEAR_SHARE
        # MUTATIONS: neither the offset of the next filter (element b + 1) nor that of the other step word explains the ancestors
        for s_, e_ in ((step, 1 + np.arange(b, dtype=np.uint64)), (1 - step, np.arange(b, dtype=np.uint64))):
            u_off = P.uniform(PC.RUN_SEED, S["UNIFORM"], s_, e_, name)
            assert not torch.equal(anc, cpu_ref.systematic(W, normalized=True, u=torch.from_numpy(u_off).reshape(b, 1)))
        if dtype == F64:
            assert differ == 0, f"move {move}: {differ} float64 ancestors differ from cpu_ref's"
            return
        for k in range(b):
            ok = P.valid_ancestor(anc[:, k].numpy(), grids[k], P.cdf64(W[:, k].numpy()), delta)
            assert ok.all(), f"move {move} filter {k}: {int((~ok).sum())} ancestors are no searchsorted of the oracle's grid within {delta:g}"

    x1, w1, anc1, ll1 = _block(filt, y, _teacher_state(filt, 3, x0, w0), 1, route, 0)
    check(1, x0, w0, anc1)
    # ... and the same run one move longer (the same draws): its second move draws its offset at step word 1, from the state the
    # one-move run ended in
    _, _, anc2, ll2 = _block(filt, y, _teacher_state(filt, 3, x0, w0), 2, route, 0)
    torch.testing.assert_close(ll2[0], ll1[0], rtol=1e-5 if dtype == F32 else 1e-12, atol=1e-5 if dtype == F32 else 1e-12)
    check(2, x1, w1, anc2)


# ---- e. own-draw mode = taped mode fed the regenerated draws -----------------------------------------------------------------------
def _context(case, dtype):
    filt = _filter(case, dtype, "systematic")
    ctx = filt._ensure_context()
    return ctx.kind, ctx.params, filt._model.hidden.n_dim > 0


def _soa_normals(seed, stream, step, n, b, d, dtype, addr_d=None):
    """``(D, B, N)`` tape in ``dtype``: the oracle's normals of element ``b N + i``, ``d`` of the ``addr_d`` numbers of an element."""
    z = PC.oracle_normals(seed, stream, step, n, b, addr_d or d, _name(dtype))[..., :d]
    return z.permute(2, 1, 0).contiguous().to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("model,n,b", [("sine", 1003, 2), ("rw2d", 1003, 2), ("lorenz", 1003, 2), ("sine", 5, 1)])
def test_sample_and_weight_own_draws(model, n, b, dtype):
    seed, step = PC.SEED_LOW, 6
    case = PC.case_of(model, "sisr", "bootstrap", n, b)
    kind, params, has_event = _context(case, dtype)
    x, _ = PC.teacher(case, dtype)
    y = PC.observations(case, dtype)[0].cuda()
    soa = ops.to_soa(x.cuda(), True, has_event)
    d = soa.shape[0]
    own_x, own_w = ops.sample_and_weight_soa(kind, params, L.PROP_BOOTSTRAP, soa, y, None, seed, step)
    z = _soa_normals(seed, S["NORMAL"], step, n, b, d, dtype).cuda()
    tap_x, tap_w = ops.sample_and_weight_soa(kind, params, L.PROP_BOOTSTRAP, soa, y, z, seed + 1, step + 1)
    err = (own_x.double() - tap_x.double()).abs().cpu()
    _say(f"pf_sample_and_weight {model} {n}x{b} {_name(dtype)}: largest |own - taped| x {float(err.max()):.3e}")
    assert bool((err <= _value_bar(dtype, tap_x.double().cpu())).all())
    if dtype == F64:
        werr = _weight_error(own_w, tap_w)
        _say(f"pf_sample_and_weight {model} {n}x{b} float64: largest |own - taped| w / (1 + |w|) {werr:.3e}")
        assert werr <= PC.VALUE_F64


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("d", [1, 2, 3, 5])
def test_initial_sample_own_draws(d, dtype):
    """Stream INIT: an element's ``D <= 3`` numbers are the first of FOUR (``D``-of-4 addressing); the planes of a ``D > 3`` state go in
    groups of three, group ``g`` at step word ``g``."""
    n, b, seed = 1003, 3, PC.SEED_LOW
    m0, s0 = [0.5 * k - 1.0 for k in range(d)], [0.25 + 0.125 * k for k in range(d)]
    z = torch.cat([_soa_normals(seed, S["INIT"], g, n, b, min(3, d - 3 * g), dtype, addr_d=4) for g in range((d + 2) // 3)], 0).cuda()
    own = ops.initial_sample_soa(m0, s0, n, b, d, dtype, torch.device("cuda"), seed)
    tap = ops.initial_sample_soa(m0, s0, n, b, d, dtype, torch.device("cuda"), seed + 1, z=z)
    err = (own.double() - tap.double()).abs().cpu()
    assert bool((err <= _value_bar(dtype, tap.double().cpu())).all()), float(err.max())
    mc = torch.tensor(m0, dtype=dtype, device="cuda").expand(b, d)
    sc = (torch.tensor(s0, dtype=dtype, device="cuda") * torch.arange(1, b + 1, dtype=dtype, device="cuda").unsqueeze(-1)).contiguous()
    own_c = ops.initial_sample_cols(mc, sc, n, b, d, seed)
    tap_c = ops.initial_sample_cols(mc, sc, n, b, d, seed + 1, z=z)
    err_c = (own_c.double() - tap_c.double()).abs().cpu() / float(b)  # (scales up to b s0)
    assert bool((err_c <= _value_bar(dtype, tap_c.double().cpu())).all()), float(err_c.max())
    _say(f"pf_initial_sample D={d} {_name(dtype)}: largest |own - taped| {float(err.max()):.3e}, per-filter rows {float(err_c.max()):.3e}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("model,m", [("sine", 1), ("sine", 5), ("sine", 16), ("rw2d", 5), ("lorenz", 5), ("lorenz", 16)])
def test_nested_own_draws(model, m, dtype):
    """Candidate ``j`` of particle ``i`` of filter ``b``: normals of element ``(b N + i) M + j`` on stream NESTED_Z, the pick from
    ``uniform(seed, NESTED_PICK, step, b N + i)``."""
    from tests import nested_cases as NC

    n, b, seed, step = 301, 2, PC.SEED_LOW, 4
    name = _name(dtype)
    call = NC.synthetic(model, n, b, m, dtype, seed=3)
    spec = build_spec(call.case, F64)
    d = max(1, spec.dim)
    elem = ((np.arange(b, dtype=np.uint64)[None, :] * np.uint64(n) + np.arange(n, dtype=np.uint64)[:, None])[None] * np.uint64(m)
            + np.arange(m, dtype=np.uint64)[:, None, None])  # (M, N, B)
    z = torch.from_numpy(P.normals(seed, S["NESTED_Z"], step, elem, d, name)).to(dtype)
    v = torch.from_numpy(P.uniform(seed, S["NESTED_PICK"], step, elem[0] // np.uint64(m), name)).to(dtype)
    regen = NC.Call(call.name + " regenerated", call.case, dtype, call.x, call.y, z if spec.dim > 0 else z[..., 0], v)
    own_x, own_w, own_pick = NC.run_kernel(call, z=False, seed=seed, step=step)
    tap_x, tap_w, tap_pick = NC.run_kernel(regen, z=True, seed=seed + 1, step=step + 1)
    differ = int((own_pick != tap_pick).sum())
    err = (own_x.double() - tap_x.double()).abs()
    _say(f"pf_nested_sample_and_weight {model} M={m} {name}: {differ} of {n * b} picks differ, largest |own - taped| x {float(err.max()):.3e}")
    assert differ == 0
    assert bool((err <= _value_bar(dtype, tap_x.double())).all())
    if dtype == F64:
        werr = _weight_error(own_w, tap_w)
        _say(f"pf_nested_sample_and_weight {model} M={m} float64: largest |own - taped| w / (1 + |w|) {werr:.3e}")
        assert werr <= PC.VALUE_F64


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("n,b", [(5003, 3), (200, 4)])  # a ragged tail (N % 4 != 0); whole groups of four
@pytest.mark.parametrize("model", ["sine", "rw2d_theta", "lorenz_o1", "lorenz_o3"])
def test_forecast_own_draws(model, n, b, dtype):
    """Transition normals: number ``(b N + i) D + d`` of stream FORECAST_Z at step word ``h``; observation noise: number
    ``(b N + i) MAXO + o`` of FORECAST_E (``MAXO`` = 1 for a scalar state, else 3) - drawn only with paths."""
    from tests import forecast_oracle as FO

    h, seed = 3, PC.SEED_LOW
    name = _name(dtype)
    inp = FO.Inputs(model, n, b, h, "random", seed=1)
    spec = build_spec(inp.case, F64)
    d, o = max(1, spec.dim), max(1, spec.obs_dim)
    maxo = 1 if d == 1 else 3
    z = torch.stack([PC.oracle_normals(seed, S["FORECAST_Z"], k, n, b, d, name) for k in range(h)], 0).to(dtype).double()
    e = torch.stack([PC.oracle_normals(seed, S["FORECAST_E"], k, n, b, maxo, name)[..., :o] for k in range(h)], 0).to(dtype).double()
    inp.z = z if inp.has_d else z[..., 0]
    inp.e = e if inp.has_o else e[..., 0]
    own = FO.run_kernel(inp, dtype, paths=True, tapes=False, seed=seed)
    tap = FO.run_kernel(inp, dtype, paths=True, tapes=True, seed=seed + 1)
    bare = FO.run_kernel(inp, dtype, paths=False, tapes=False, seed=seed)  # without paths: the same transition draws
    bar = PC.VALUE_F64 if dtype == F64 else PC.NORMAL_F32  # (of 1 + |value|: ``scaled_error``)
    worst = {k: FO.scaled_error(own[k], tap[k].cpu()) for k in FO.KEYS}
    _say(f"pf_forecast {model} {n}x{b} H={h} {name}: largest scaled |own - taped| " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= bar, worst
    for k in ("x_mean", "x_var", "y_mean", "y_var"):
        assert FO.scaled_error(bare[k], own[k].cpu()) <= (1e-12 if dtype == F64 else 1e-5), k


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("model,n,b", [("sine", 257, 2), ("rw2d", 257, 2), ("lorenz", 1537, 3)])
def test_ffbs_own_draws(model, n, b, dtype):
    """One backward draw: trajectory ``j`` of filter ``b`` takes ``uniform(seed, SMOOTH, t, b N + j)`` - exact in either type, so the
    taped call on the regenerated uniforms returns the same particles bit for bit."""
    from tests import smoothing_cases as SC

    seed, name = PC.SEED_LOW, _name(dtype)
    hist = SC.synthetic(model, n, b, 2, dtype)
    kind, params = hist.context()
    x_hist, logw, x_last, _ = hist.soa()
    own = ops.smooth_ffbs(kind, params, x_hist, logw, x_last, None, seed)
    u = np.stack([P.uniform(seed, S["SMOOTH"], 0, k * n + np.arange(n, dtype=np.uint64), name) for k in range(b)])[None]  # (1, B, N)
    tap = ops.smooth_ffbs(kind, params, x_hist, logw, x_last, torch.from_numpy(u).to(dtype).cuda(), seed + 1)
    assert torch.equal(own, tap), f"{int((own != tap).any(dim=1).sum())} backward draws differ from the taped call"
    # MUTATION: the uniforms of step word 1 must give other draws
    other = np.stack([P.uniform(seed, S["SMOOTH"], 1, k * n + np.arange(n, dtype=np.uint64), name) for k in range(b)])[None]
    assert not torch.equal(own, ops.smooth_ffbs(kind, params, x_hist, logw, x_last, torch.from_numpy(other).to(dtype).cuda(), seed))
    _say(f"pf_smooth_ffbs {model} {n}x{b} {name}: own draws = taped draws, bit for bit")
