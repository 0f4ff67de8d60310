from . import proposals
from .apf import APF
from .base import ParticleFilter
from .forecast import Forecast, mix_forecasts
from .sisr import SISR

__all__ = ["proposals", "APF", "SISR", "ParticleFilter", "Forecast", "mix_forecasts"]
