"""Drop-in for the reference's variance_learner.py (jsrl_utils.py:15 imports StateDepFunction and VarianceLearner from
it): the implementation is iqlhip_variance.py, whose gradient step runs on the GPU.  StateActionVarianceLearner and
test_model are not ported (iqlhip_variance.py: why).  Beyond the reference's surface, VarianceLearner trains from a
GPU replay buffer (pack_window, update_from_buffer, get_values_window, train_on_buffer, run_training_on_buffer;
TRAIN_MAX_STEPS updates per library call), and VarianceLearnerGroup does all of that for up to MAX_GROUP learners with
one set of launches per update."""
from iqlhip_variance import (GAMMA, MAX_GROUP, TRAIN_MAX_STEPS, StateDepFunction, VarianceLearner,  # noqa: F401
                             VarianceLearnerGroup, mse_loss, nll_loss, pack_block, run_episodes, to_tensor)

__all__ = ["GAMMA", "MAX_GROUP", "TRAIN_MAX_STEPS", "StateDepFunction", "VarianceLearner", "VarianceLearnerGroup", "mse_loss",
           "nll_loss", "pack_block", "run_episodes", "to_tensor"]
