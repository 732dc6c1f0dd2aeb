"""Drop-in for the reference's variance_learner.py (jsrl_utils.py:15 imports StateDepFunction and VarianceLearner from
it): the implementation is iqlhip_variance.py, whose gradient step runs on the GPU.  StateActionVarianceLearner and
test_model are not ported (iqlhip_variance.py: why)."""
from iqlhip_variance import (GAMMA, StateDepFunction, VarianceLearner, mse_loss, nll_loss, run_episodes,  # noqa: F401
                             to_tensor)

__all__ = ["GAMMA", "StateDepFunction", "VarianceLearner", "mse_loss", "nll_loss", "run_episodes", "to_tensor"]
