"""Plain restatement of the JSRL host rules the tests compare against: the horizon functions' decision for one state
(time_step, goal_dist, variance, agent_type) and jsrl_w_iql.eval_actor for one member with callables as policies."""
import numpy as np

ACCUMULATE = {"time_step": np.mean, "agent_type": lambda v: 1, "goal_dist": np.max, "variance": np.mean}


def horizon_decision(fn, step, cfg, value=None):
    """(use_learner, horizon) of one horizon function.  `value`: the goal distance or the variance."""
    nan = bool(np.isnan(cfg.curriculum_stage))
    last = cfg.curriculum_stage_idx == cfg.n_curriculum_stages - 1
    if fn == "agent_type":
        if nan:
            return True, cfg.ep_agent_type
        use = False
        if last or cfg.ep_agent_type <= cfg.curriculum_stage:
            use = bool(np.random.sample() < cfg.curriculum_stage)
        return use, cfg.ep_agent_type
    h = step if fn == "time_step" else value
    if nan:
        return True, h
    reached = (step >= cfg.curriculum_stage) if fn == "time_step" else (h <= cfg.curriculum_stage)
    return bool((reached or last) and cfg.ep_agent_type <= cfg.agent_type_stage), h


def eval_member(env, learner, guide, cfg, fn, n_episodes, seed, value_fn=None):
    """eval_actor for one member: learner(state) / guide(state) return actions, value_fn(state, env) the goal distance
    or the variance.  guide None: the learner always acts."""
    env.seed(seed)
    rewards, successes, horizons, types = [], [], [], []
    for _ in range(n_episodes):
        state, done = env.reset(), False
        ts, total, ep_h, ep_t, ok = 0, 0.0, [], [], False
        while not done:
            cfg.ep_agent_type = 0 if ts == 0 else np.mean(ep_t)
            use, h = horizon_decision(fn, ts, cfg, None if value_fn is None else value_fn(state, env))
            if guide is None:
                use = True
            action = learner(state) if use else guide(state)
            ep_h.append(h)
            ep_t.append(1 if use else 0)
            state, reward, done, info = env.step(action)
            total += reward
            ts += 1
            if not ok:
                ok = info["success"] if "success" in info else reward > 0
        successes.append(float(ok))
        rewards.append(total)
        horizons.append(np.max(ep_h) if (guide is None and cfg.max_init_horizon) else ACCUMULATE[fn](ep_h))
        types.append(np.mean(ep_t))
    top = guide is None and cfg.max_init_horizon
    return np.asarray(rewards), np.mean(successes), (np.max(horizons) if top else np.mean(horizons)), np.mean(types)
