"""TEST INFRASTRUCTURE - what the NESS replays share (``tests/test_ness_cpu.py``: the product's torch route on the oracle-backed
CPU stand-in filter; ``tests/test_ness_gpu.py``: both theta routes on the HIP filters): the event logs
``tests/golden/inference_ness_*.npz`` (written by ``tools/make_golden_ness.py`` from the unmodified reference's ``NESS`` /
``FixedWidthNESS`` / ``OnlineKernel`` / jittering kernels) are driven through ``pyfilter_amd.inference.NESS.step``: every random
number the reference consumed is handed to the product at the same point - a product that updates at another observation, or
draws in another order, fails on the event kinds - and every quantity the reference computed is compared on the way."""
import torch

from pyfilter_amd.inference.ness import NessDraws
from tests.replay import Cursor, close, load_events

CONSTANT_SCALE = 0.05  # tools/make_golden_ness.py
NESS_CASES = {
    "inference_ness_ou": dict(B=40, N=64, alg="ness", kernel="nonshrinking", discrete=False, kwargs=dict(threshold=0.9)),
    "inference_ness_ou_shrink": dict(B=32, N=64, alg="ness", kernel="shrinking", discrete=False, kwargs=dict(threshold=0.9)),
    "inference_ness_ou_liuwest": dict(B=32, N=64, alg="ness", kernel="liuwest", discrete=False, kwargs=dict(threshold=0.9)),
    "inference_ness_ou_const": dict(B=24, N=64, alg="ness", kernel="constant", discrete=True, kwargs=dict(threshold=0.9)),
    "inference_ness_ou_fixed": dict(B=16, N=64, alg="fixed", kernel="nonshrinking", discrete=False, kwargs=dict(block_len=5)),
}


def make_kernel(name):
    from pyfilter_amd.inference import ConstantKernel, LiuWestShrinkage, NonShrinkingKernel, ShrinkingKernel

    return {"nonshrinking": NonShrinkingKernel, "shrinking": ShrinkingKernel, "liuwest": LiuWestShrinkage,
            "constant": lambda: ConstantKernel(torch.tensor(CONSTANT_SCALE, dtype=torch.float64))}[name]()


class NessReplayDraws(NessDraws):
    """The theta-level draws of an update in the reference's order, all out of ONE ``jitter`` event: the resampling uniform
    (``online.py:33``) opens it, then the standard normals (``jittering.py:26``), then - ``discrete`` - the Bernoulli draws
    (``online.py:39-43``).  ``taped``: the kernel route takes them too instead of drawing on the device."""

    taped = True

    def __init__(self, cursor: Cursor):
        self.cursor, self.generator, self.event, self.given = cursor, None, None, []

    def uniform(self, shape):
        assert tuple(shape) == (), shape
        self.event, self.given = self.cursor.take("jitter"), ["u"]
        return self.event["u"].double().reshape(())

    def _next(self, field, after, shape):
        assert self.event is not None and self.given == after, f"'{field}' asked after {self.given}: the reference draws it after {after}"
        assert field in self.event, f"the reference drew no '{field}' in this update"
        self.given.append(field)
        v = self.event[field].double()
        assert tuple(v.shape) == tuple(shape), (field, v.shape, shape)
        return v

    def normal(self, shape):
        return self._next("eps", ["u"], shape)

    def bernoulli(self, shape, p):
        assert abs(p - shape[0] ** -0.5) < 1e-15, p
        return self._next("bernoulli", ["u", "eps"], shape)


def priors():
    from torch.distributions import Exponential, LogNormal, Normal

    return {"kappa": Exponential(10.0), "gamma": Normal(0.0, 1.0), "sigma": LogNormal(-2.0, 1.0)}  # tests/inference/models.py:29-31


def replay_ness(name, make_filter, device, rtol=1e-8):
    """Drives ``NESS.step`` / ``FixedWidthNESS.step`` over the fixture's observations; returns (updates compared, the routes
    they took)."""
    from pyfilter_amd.inference import NESS, FixedWidthNESS

    case = NESS_CASES[name]
    events = load_events(name)
    cur = Cursor(events)
    head = cur.take("theta0")
    y = head["y"].to(device)
    filt = make_filter(cur, case["N"])
    cls = NESS if case["alg"] == "ness" else FixedWidthNESS
    alg = cls(filt, case["B"], priors(), kernel=make_kernel(case["kernel"]), discrete=case["discrete"], device=device,
              dtype=torch.float64, **case["kwargs"])
    draws = alg._gen = NessReplayDraws(cur)
    online = alg._kernel
    online.trace = []
    after = []
    real_update = online.update

    def update(theta, filter_, state, generator=None):  # (what the update left, before the move of the same step changes it)
        out = real_update(theta, filter_, state, generator=generator)
        after.append(dict(theta=theta.stack_parameters(True).clone(), w=out.w.clone(), ll=out.filter_state.loglikelihood.clone()))
        return out

    online.update = update
    state = alg.initialize(theta0=head["theta"])
    close(alg.theta.stack_parameters(True), head["theta"], "theta0")
    updates, routes = 0, set()
    for t in range(y.shape[0]):
        at = cur.at
        due = events[at][0] == "jitter"
        state = alg.step(y[t], state)
        assert len(online.trace) == len(after) == (1 if due else 0), f"t={t}: the reference {'updates' if due else 'does not update'} here"
        if due:
            ev, tr, left = events[at][1], online.trace.pop(), after.pop()
            what = f"{name} t={t}"
            assert draws.given == ["u", "eps"] + (["bernoulli"] if case["discrete"] else []), (what, draws.given)
            assert torch.equal(tr["indices"].cpu(), ev["indices"]), f"{what}: theta ancestors"
            if "mean" in tr:  # (the kernel route never forms the (B, P) locations: they are pinned through `jittered` below)
                close(tr["mean"], ev["mean"], f"{what}: fit mean")
            close(tr["scale"], ev["scale"].expand(tr["scale"].shape), f"{what}: fit scale")
            close(tr["std"], ev["std"].expand(tr["std"].shape), f"{what}: clamped std")
            close(tr["jittered"], ev["jittered"], f"{what}: jittered theta (unconstrained)")
            close(left["theta"], ev["theta"], f"{what}: jittered theta (constrained)")
            close(left["w"], ev["w"], f"{what}: theta-weights after the update")
            close(left["ll"], ev["ll"], f"{what}: the gathered filters' log-likelihoods", rtol=rtol)
            routes.add(tr["route"])
            updates += 1
            at += 1
        mv = events[at][1]
        assert events[at][0] == "move" and cur.at == at + 1
        close(filt.last_move_ll, mv["ll"], f"t={t}: log-likelihood increments", rtol=rtol)
        close(state.ess[t + 1], mv["ess_after"], f"t={t}: ESS of the theta-weights", rtol=rtol)
    fin = cur.take("final")
    assert cur.peek() is None
    close(state.filter_state.filter_means, fin["filter_means"], "filter means of the whole run", rtol=1e-7, atol=1e-9)
    close(state.filter_state.filter_variance, fin["filter_variance"], "filter variances", rtol=1e-6, atol=1e-10)
    close(state.filter_state.loglikelihood, fin["ll"], "log-likelihoods", rtol=rtol)
    close(state.w, fin["w"], "theta-weights", rtol=rtol)
    close(torch.stack(state.ess), fin["ess"], "ESS history", rtol=rtol)
    close(alg.theta.stack_parameters(True), fin["theta"], "theta")
    assert updates == sum(k == "jitter" for k, _ in events)
    return updates, routes
