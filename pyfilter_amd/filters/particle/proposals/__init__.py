from .base import Proposal
from .bootstrap import Bootstrap
from .linear import LinearGaussianObservations
from .nested import NestedProposal

__all__ = ["Proposal", "Bootstrap", "LinearGaussianObservations", "NestedProposal"]
