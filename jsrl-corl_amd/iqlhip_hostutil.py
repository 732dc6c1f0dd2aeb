"""Host-side helpers the reference's loops import from `iql`
(jsrl_w_iql.py:24-41, jsrl_utils.py:16-22): dataset normalisation, reward
shaping, env wrapping, seeding.  Pure numpy / python, no device work.
gym / gymnasium / wandb are imported lazily: they are host-only and absent on
the GPU box.
"""
from __future__ import annotations

import os
import random
import uuid
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

ENVS_WITH_GOAL = ("antmaze", "pen", "door", "hammer", "relocate", "Adroit")
_LOCOMOTION = ("halfcheetah", "hopper", "walker2d")


def soft_update(target: nn.Module, source: nn.Module, tau: float):
    """Polyak averaging on modules (iql.py:72-74); the trainer does this inside the fused
    update kernel, this function exists for callers that import it."""
    with torch.no_grad():
        for t, s in zip(target.parameters(), source.parameters()):
            t.data.copy_((1 - tau) * t.data + tau * s.data)


def compute_mean_std(states: np.ndarray, eps: float) -> Tuple[np.ndarray, np.ndarray]:
    return states.mean(0), states.std(0) + eps


def normalize_states(states: np.ndarray, mean: np.ndarray, std: np.ndarray):
    return (states - mean) / std


def wrap_env(env, state_mean: Union[np.ndarray, float] = 0.0, state_std: Union[np.ndarray, float] = 1.0,
             reward_scale: float = 1.0):
    """Observation normalisation / reward scaling wrappers (iql.py:87-119), including the
    reference's handling of gymnasium's (obs, info) tuples as written there."""

    def normalize_state(state):
        info = None
        if isinstance(state, tuple):
            state = state[0]
            info = state[1]   # (sic) mirrors the reference, SURVEY Appendix A
        state = (state - state_mean) / state_std
        return state if info is None else (state, info)

    def scale_reward(reward):
        return reward_scale * reward

    if "gymnasium" in str(type(env)):
        import gymnasium
        env = gymnasium.wrappers.TransformObservation(env, normalize_state, env.observation_space)
        if reward_scale != 1.0:
            env = gymnasium.wrappers.TransformReward(env, scale_reward)
    else:
        import gym
        env = gym.wrappers.TransformObservation(env, normalize_state)
        if reward_scale != 1.0:
            env = gym.wrappers.TransformReward(env, scale_reward)
    return env


def set_env_seed(env, seed: int):
    env.seed(seed)
    env.action_space.seed(seed)


def set_seed(seed: int, env=None, deterministic_torch: bool = False):
    if env is not None:
        set_env_seed(env, seed)
    os.environ["PYTHONHASHSEED"] = str(seed)
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)
    torch.use_deterministic_algorithms(deterministic_torch)


def wandb_init(config: dict) -> None:
    import wandb
    wandb.init(config=config, project=config["project"], group=config["group"], name=config["name"],
               id=str(uuid.uuid4()))
    wandb.run.save()


def is_goal_reached(reward: float, info: Dict) -> bool:
    for key in ("goal_achieved", "success"):
        if key in info:
            return info[key]
    return reward > 0


@torch.no_grad()
def eval_actor(env, actor: nn.Module, device: str, n_episodes: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    env.seed(seed)
    actor.eval()
    returns, successes = [], []
    for _ in range(n_episodes):
        state, done = env.reset(), False
        total, reached = 0.0, False
        while not done:
            state, reward, done, infos = env.step(actor.act(state, device))
            total += reward
            reached = reached or is_goal_reached(reward, infos)
        successes.append(float(reached))
        returns.append(total)
    actor.train()
    return np.asarray(returns), np.mean(successes)


def _group_for(actors, device):
    """The trainer group that can act for `actors` on `device` (their owning trainers, two or more, distinct, a valid
    GPU group), else None.  Valid means the library accepts the group too: its rules are checked on the contexts, e.g.
    a member whose last training step ran with actor dropout keeps that dropout rate in its context and is refused
    even while its actor is in eval mode."""
    if len(actors) < 2:
        return None
    from iqlhip_group import ImplicitQLearningGroup
    from iqlhip_networks import _hip_owner
    owners = [_hip_owner(a, device) for a in actors]
    if any(o is None or o.actor is not a for o, a in zip(owners, actors)):
        return None
    try:
        group = ImplicitQLearningGroup(owners)
        group._group()          # the library group now, so that its refusal selects the per-actor path
    except (ValueError, RuntimeError, NotImplementedError):
        return None
    return group


@torch.no_grad()
def eval_actors(envs, actors, device: str, n_episodes: int, seeds) -> List[Tuple[np.ndarray, np.ndarray]]:
    """eval_actor(envs[k], actors[k], device, n_episodes, seeds[k]) for every k, in lockstep: each round steps every
    member still inside its episodes, with one group act() for all of them when the actors' trainers form a GPU
    group (else — and for a round with one member left — per-actor act() calls in member order: the same results).  Each env sees exactly eval_actor's call
    sequence (seed, reset, step, ...); a member whose episodes are done drops out of later rounds."""
    envs, actors, seeds = list(envs), list(actors), list(seeds)
    K = len(actors)
    if len(envs) != K or len(seeds) != K:
        raise ValueError(f"eval_actors: {len(envs)} envs, {K} actors and {len(seeds)} seeds (one each)")
    for env, seed in zip(envs, seeds):
        env.seed(seed)
    for a in actors:
        a.eval()
    group = _group_for(actors, device)
    returns = [[] for _ in range(K)]
    successes = [[] for _ in range(K)]
    state, total, reached = [None] * K, [0.0] * K, [False] * K
    live = [k for k in range(K) if n_episodes > 0]
    for k in live:
        state[k] = envs[k].reset()
    try:
        while live:
            if group is not None and len(live) > 1:
                acts = group.act([state[k] if k in live else None for k in range(K)])
            else:
                acts = [actors[k].act(state[k], device) if k in live else None for k in range(K)]
            still = []
            for k in live:
                state[k], reward, done, infos = envs[k].step(acts[k])
                total[k] += reward
                reached[k] = reached[k] or is_goal_reached(reward, infos)
                if done:
                    successes[k].append(float(reached[k]))
                    returns[k].append(total[k])
                    if len(returns[k]) == n_episodes:
                        continue
                    state[k], total[k], reached[k] = envs[k].reset(), 0.0, False
                still.append(k)
            live = still
    finally:
        if group is not None:
            group._release()
    for a in actors:
        a.train()
    return [(np.asarray(returns[k]), np.mean(successes[k])) for k in range(K)]


# the reference's accumulator of an episode's horizons, per horizon function (jsrl_utils.HORIZON_FNS)
_JSRL_ACCUMULATORS = {"time_step": np.mean, "agent_type": lambda v: 1, "goal_dist": np.max, "variance": np.mean}


@torch.no_grad()
def eval_actors_jsrl(envs, jsrl, configs, horizon_fn: str, n_episodes: int, seeds, goal_dist=None, who=None,
                     q_inv_temp=None):
    """jsrl_w_iql.eval_actor (guide and learner mixed per step) for every member of `jsrl` in lockstep, on ONE
    jsrl.act per round: returns per member (episode returns, mean success, horizon, mean agent type).  configs[k] is
    the member's JsrlTrainConfig; its ep_agent_type is maintained as the reference does (0 at an episode's first step,
    then the mean of the episode's choices so far); the episode horizons are accumulated with the reference's
    accumulator of `horizon_fn` — or, for a member without a guide and config.max_init_horizon, with max.  The
    `variance` horizon is the gate's value, compared on the device with config.curriculum_stage.
    who: None, or per member None (the horizon rule decides) or a byte that replaces the rule's at every step — 3, the
    member's critic picks (JsrlActors(..., critics=...)), is written this way: the horizon rules never produce it.
    q_inv_temp goes to jsrl.act as it is."""
    from iqlhip_jsrl import who_from_config
    envs, configs, seeds = list(envs), list(configs), list(seeds)
    K = len(envs)
    fixed = [None] * K if who is None else list(who)
    if len(fixed) != K:
        raise ValueError(f"eval_actors_jsrl: who needs one entry per member ({K})")
    more = {} if q_inv_temp is None else {"q_inv_temp": q_inv_temp}
    if len(configs) != K or len(seeds) != K or len(jsrl.learners) != K:
        raise ValueError(f"eval_actors_jsrl: {K} envs, {len(configs)} configs, {len(seeds)} seeds and "
                         f"{len(jsrl.learners)} JSRL members (one each)")
    accumulate = _JSRL_ACCUMULATORS[horizon_fn] if horizon_fn in _JSRL_ACCUMULATORS else None
    if accumulate is None:
        raise ValueError(f"eval_actors_jsrl: unknown horizon function {horizon_fn!r}")
    for env, seed in zip(envs, seeds):
        env.seed(seed)
    jsrl.eval()
    no_guide = [jsrl.guides[k] is None and bool(getattr(configs[k], "max_init_horizon", False)) for k in range(K)]
    returns, successes, horizons, agent_types = ([[] for _ in range(K)] for _ in range(4))
    state, ts, total, reached = [None] * K, [0] * K, [0.0] * K, [False] * K
    ep_h, ep_types = [[] for _ in range(K)], [[] for _ in range(K)]
    live = [k for k in range(K) if n_episodes > 0]
    for k in live:
        state[k] = envs[k].reset()
    while live:
        for k in live:
            configs[k].ep_agent_type = 0 if ts[k] == 0 else np.mean(ep_types[k])
        who_k, hz = who_from_config([configs[k] for k in live], horizon_fn, [ts[k] for k in live],
                                  [state[k] for k in live], [envs[k] for k in live], goal_dist=goal_dist)
        who_all, gate_max = [None] * K, [0.0] * K
        for j, k in enumerate(live):
            who_all[k] = who_k[j] if fixed[k] is None else np.array([fixed[k]], dtype=np.int8)
            stage = configs[k].curriculum_stage
            gate_max[k] = 0.0 if np.isnan(stage) else float(stage)
        got = jsrl.act([state[k] if k in live else None for k in range(K)], who_all, gate_max, **more)
        still = []
        for j, k in enumerate(live):
            acts, use, h = got[k][:3]
            action, use_learner = acts[0], bool(use[0])
            if getattr(configs[k], "discrete", False) and use_learner and jsrl.guides[k] is not None:
                action = np.argmax(action)
            ep_h[k].append(hz[j] if hz[j] is not None else h[0])
            ep_types[k].append(1 if use_learner else 0)
            state[k], reward, done, infos = envs[k].step(action)
            total[k] += reward
            ts[k] += 1
            reached[k] = reached[k] or is_goal_reached(reward, infos)
            if done:
                successes[k].append(float(reached[k]))
                returns[k].append(total[k])
                horizons[k].append(np.max(ep_h[k]) if no_guide[k] else accumulate(ep_h[k]))
                agent_types[k].append(np.mean(ep_types[k]))
                if len(returns[k]) == n_episodes:
                    continue
                state[k], ts[k], total[k], reached[k] = envs[k].reset(), 0, 0.0, False
                ep_h[k], ep_types[k] = [], []
            still.append(k)
        live = still
    jsrl.train()
    return [(np.asarray(returns[k]), np.mean(successes[k]),
             (np.max(horizons[k]) if no_guide[k] else np.mean(horizons[k])) if horizons[k] else np.nan,
             np.mean(agent_types[k])) for k in range(K)]


def return_reward_range(dataset: Dict, max_episode_steps: int) -> Tuple[float, float]:
    """min / max episode return of a D4RL dataset (semantics of iql.py:262-274): an episode ends at a terminal
    flag or after max_episode_steps steps, whichever comes first; a trailing unfinished episode is not counted.
    Episode boundaries are found per terminal-delimited run (a 1 M-row locomotion dataset has ~1 k of them), the
    returns with one segmented float64 sum — no per-transition Python loop."""
    rewards = np.asarray(dataset["rewards"], dtype=np.float64).reshape(-1)
    n = rewards.shape[0]
    term_at = np.flatnonzero(np.asarray(dataset["terminals"]).reshape(-1).astype(bool))
    run_first = np.concatenate(([0], term_at + 1))
    run_stop = np.concatenate((term_at + 1, [n]))                  # exclusive
    pieces = []
    for i, (lo, hi) in enumerate(zip(run_first.tolist(), run_stop.tolist())):
        if hi <= lo:
            continue
        cuts = np.arange(lo + max_episode_steps - 1, hi, max_episode_steps)      # time-limit ends inside the run
        if i < term_at.shape[0] and (cuts.size == 0 or cuts[-1] != hi - 1):
            cuts = np.append(cuts, hi - 1)                                        # the run's terminal step
        pieces.append(cuts)
    last = np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.int64)
    if last.size == 0:
        raise ValueError("min() arg is an empty sequence")        # what the reference's min(returns) raises
    first = np.concatenate(([0], last[:-1] + 1))
    returns = np.add.reduceat(np.append(rewards, 0.0), np.append(first, last[-1] + 1))[:-1]
    return float(returns.min()), float(returns.max())


def modify_reward(dataset: Dict, env_name: str, max_episode_steps: int = 1000) -> Dict:
    if any(s in env_name for s in _LOCOMOTION):
        min_ret, max_ret = return_reward_range(dataset, max_episode_steps)
        dataset["rewards"] /= max_ret - min_ret
        dataset["rewards"] *= max_episode_steps
        return {"max_ret": max_ret, "min_ret": min_ret, "max_episode_steps": max_episode_steps}
    if "antmaze" in env_name:
        dataset["rewards"] -= 1.0
    return {}


def modify_reward_online(reward: float, env_name: str, **kwargs) -> float:
    if any(s in env_name for s in _LOCOMOTION):
        reward /= kwargs["max_ret"] - kwargs["min_ret"]
        reward *= kwargs["max_episode_steps"]
    elif "antmaze" in env_name:
        reward -= 1.0
    return reward


def asymmetric_l2_loss(u: torch.Tensor, tau: float) -> torch.Tensor:
    """Expectile loss (iql.py:301-302); the trainer computes it inside the backward kernel."""
    return torch.mean(torch.abs(tau - (u < 0).float()) * u ** 2)
