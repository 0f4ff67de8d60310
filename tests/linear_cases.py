"""Shared by the linear-model tests: the fixtures of ``tools/make_golden_linear.py`` (models of 4 to 8 state components, recorded
from the unmodified reference) and the product-side models rebuilt from the parameters each fixture carries."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name: (filter, proposal, ESS threshold, float32 fixture too)
CASES = {
    "cv4d_sisr_boot": ("sisr", "bootstrap", 0.7, True),
    "cv4d_apf_lgo": ("apf", "lgo", 0.7, True),
    "lm6d_sisr_lgo": ("sisr", "lgo", 0.7, False),
    "lm8d_apf_boot": ("apf", "bootstrap", 0.7, False),
    "rw5d_sisr_lgo": ("sisr", "lgo", 0.7, False),
}
PARAMS = [(n, "f64") for n in CASES] + [(n, "f32") for n, c in CASES.items() if c[3]]
DT = {"f64": torch.float64, "f32": torch.float32}


def load(name, dt):
    with np.load(os.path.join(GOLDEN, f"{name}_{dt}.npz")) as f:
        return {k: torch.from_numpy(f[k]) for k in f.files}


def build_ssm(name, g, dtype, device, how="model"):
    """``how``: ``"model"`` - ``LinearModel`` (``RandomWalk(dim=5)`` for the walk); ``"lambda"`` - the same model as a plain
    ``AffineProcess`` lambda (no kernel kind at these dimensions: torch model arithmetic)."""
    from torch.distributions import Independent, Normal

    from pyfilter_amd import timeseries as ts
    from pyfilter_amd.timeseries import models

    p = {k: g[k].to(device=device, dtype=dtype) for k in ("hid_A", "hid_b", "hid_s", "obs_A", "obs_b", "obs_s", "init_m", "init_s")}
    d, o = p["hid_A"].shape[0], p["obs_A"].shape[0]
    m0, s0 = p["init_m"], p["init_s"]

    def init_kernel(*_):
        return Independent(Normal(m0, s0), 1)

    inc = Independent(Normal(torch.tensor(0.0, device=device, dtype=dtype), torch.tensor(1.0, device=device, dtype=dtype))
                      .expand(torch.Size([d])), 1)
    params = (p["hid_A"], p["hid_b"], p["hid_s"])
    if how == "lambda":
        hidden = ts.AffineProcess(lambda x, a, b, s: (b + (a @ x.value.unsqueeze(-1)).squeeze(-1), s), params, inc, init_kernel)
    elif name.startswith("rw5d"):
        hidden = models.RandomWalk(p["hid_s"], initial_mean=m0, initial_scale=s0, dim=d)
    else:
        hidden = models.LinearModel(params, inc, init_kernel)
    return ts.LinearStateSpaceModel(hidden, (p["obs_A"], p["obs_b"], p["obs_s"]), torch.Size([o]))


def build_filter(name, g, dtype, device, how="model", tape=True, **kwargs):
    from pyfilter_amd.filters.particle import APF, SISR, proposals

    filt_name, prop_name, ess, _ = CASES[name]
    ssm = build_ssm(name, g, dtype, device, how)
    prop = {"bootstrap": proposals.Bootstrap, "lgo": proposals.LinearGaussianObservations}[prop_name]()
    cls = {"sisr": SISR, "apf": APF}[filt_name]
    n, b = g["x0"].shape[0], g["x0"].shape[1]
    filt = cls(ssm, n, proposal=prop, ess_threshold=ess, **kwargs)
    filt.set_batch_shape(torch.Size([b]))
    if tape:
        filt.set_tape(z=g["z_tape"].to(dtype), u=g["u_tape"].to(dtype), z0=g["z0"].to(dtype))
    return filt


def start_at_x0(filt, g, device):
    """The filter's initial state with the reference's recorded initial particles (a ``LinearModel``'s initial kernel is the
    user's own distribution: its draw is torch's, not a tape's)."""
    state = filt.initialize()
    state["_x"] = state["_x"].copy(values=g["x0"].to(device=device, dtype=state["_x"].value.dtype).contiguous())
    for k in ("_mean", "_var"):
        if k in state:
            del state[k]
    return state
