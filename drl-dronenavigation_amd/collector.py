"""Rollout collection over sharded drones: the host loop around the step kernel for BASELINE configs 3-5.

What it stands in for in the reference: SB3 `OnPolicyAlgorithm.collect_rollouts` driving the
`SubprocVecEnv` built at Sol/Model/PBDroneSimulator.py:653-666 (policy -> clip -> env.step -> buffer.add,
then `compute_returns_and_advantage`), whose only in-tree statement of the advantage recursion is
Sol/Model/Algorithms/cleanRLPPO.py:207-248.  Here every buffer stays on the GPU: the policy's output tensor is
handed to `dn_step` by pointer, the rollout is laid out step-major [n_steps, N_local, ...] and the advantages
come from the `dn_gae` kernel.

Sharding: every drone is an independent world, so rank r of R owns the contiguous range
[r*N_local, (r+1)*N_local) and stepping needs NO collective.  The one exchange is per rollout: where the
learner draws its minibatches from the global batch (BASELINE config 4) the packed [2, n_steps, N_local]
advantages/returns are all-gathered (RCCL `ncclAllGather` over xGMI when the process group's backend is
"nccl"; the same call runs on gloo for the CPU tests).

`ShardPlan` and `all_gather_rollout` are device-agnostic (plain torch.distributed); `RolloutCollector` needs
the HIP environment and has no CPU path.
"""
from dataclasses import dataclass

import torch


@dataclass(frozen=True)
class ShardPlan:
    """Contiguous split of `global_num_envs` drones over `world_size` ranks."""
    global_num_envs: int
    world_size: int
    rank: int

    def __post_init__(self):
        if self.world_size < 1 or not 0 <= self.rank < self.world_size:
            raise ValueError(f"bad rank/world_size {self.rank}/{self.world_size}")
        if self.global_num_envs < self.world_size or self.global_num_envs % self.world_size:
            raise ValueError(f"global_num_envs ({self.global_num_envs}) must be a positive multiple of the world size "
                             f"({self.world_size}): all_gather_into_tensor needs equal shards")

    @property
    def num_envs(self):
        """Drones owned by this rank."""
        return self.global_num_envs // self.world_size

    @property
    def env_id_offset(self):
        """Global id of this rank's drone 0 (keys the Philox noise streams; dn_config.env_id_offset)."""
        return self.rank * self.num_envs

    def local_slice(self):
        return slice(self.env_id_offset, self.env_id_offset + self.num_envs)

    @classmethod
    def from_env(cls, global_num_envs):
        import os
        return cls(int(global_num_envs), int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")))


def all_gather_rollout(advantages, returns, group=None):
    """All-gather the per-rank [n_steps, N_local] advantages and returns into [n_steps, N_global] tensors whose
    columns are in global drone order.  One collective for both arrays (packed [2, T, N_local] send buffer ->
    [R*2, T, N_local] receive buffer), none at all without a process group (a one-rank group still goes through the
    collective, which keeps that code path testable on one GPU).  Convenience form: it allocates the receive buffer and a
    permuted copy on every call; a collector that gathers every rollout uses RolloutGather below, which does neither."""
    import torch.distributed as dist
    if advantages.shape != returns.shape or advantages.dim() != 2:
        raise ValueError("advantages and returns must both be [n_steps, N_local]")
    if not (dist.is_available() and dist.is_initialized()):
        return advantages, returns
    world = dist.get_world_size(group)
    T, n = advantages.shape
    send = torch.stack((advantages, returns)).contiguous()                       # [2, T, n]
    recv = torch.empty((world * 2, T, n), dtype=send.dtype, device=send.device)     # concatenated along dim 0
    dist.all_gather_into_tensor(recv, send, group=group)
    out = recv.view(world, 2, T, n).permute(1, 2, 0, 3).reshape(2, T, world * n)   # rank-major columns = global order
    return out[0], out[1]


class RolloutGather:
    """The per-rollout exchange of BASELINE config 4 with every buffer allocated ONCE: `send` [2, T, N_local] is the storage the
    collector's advantages / returns live in (`advantages = send[0]`, `returns = send[1]`: dn_gae writes straight into the send
    buffer, no packing copy), `recv` [R, 2, T, N_local] is what `all_gather_into_tensor` fills, and the global arrays are
    returned as strided VIEWS of it, shaped [T, R, N_local]: element [t, r, i] belongs to global drone r * N_local + i (rank-major
    = global drone order), so `view.reshape(T, R * N_local)` is the [n_steps, N_global] array where a consumer needs it flat.
    67 MB per rollout at R = 8, n_steps = 32, 32 768 drones per rank: neither allocated nor copied per rollout.
    Without a process group gather() returns the local arrays as [T, 1, N_local] views (no collective)."""

    def __init__(self, n_steps, num_envs, device, group=None, dtype=torch.float32):
        import torch.distributed as dist
        self.group = group
        self.active = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if self.active else 1
        self.send = torch.zeros((2, int(n_steps), int(num_envs)), dtype=dtype, device=device)
        self.recv = torch.zeros((self.world, 2, int(n_steps), int(num_envs)), dtype=dtype, device=device) if self.active else None

    advantages = property(lambda self: self.send[0])
    returns = property(lambda self: self.send[1])

    def gather(self):
        if not self.active:
            return self.send[0].unsqueeze(1), self.send[1].unsqueeze(1)
        import torch.distributed as dist
        dist.all_gather_into_tensor(self.recv.view(self.world * 2, *self.send.shape[1:]), self.send, group=self.group)
        return self.recv[:, 0].permute(1, 0, 2), self.recv[:, 1].permute(1, 0, 2)      # [T, R, n] views, no copy


# What the fused collectors do not carry: (env attribute, the rest of the message), refused in this order.  They evaluate actor and critic
# in one launch over the 13-column observation their step path hands on, straight from the step kernel's own output: the privileged and
# goal rows are written by other kernel families, which carry no sampling-fused entry point (a track bank rides in the goal family), and
# the history rows are stacked by a kernel of their own, after the step.
_EXTRA_ROWS = (
    ("privileged", "privileged observations (its step path shows actor and critic the same 13-column observation); "
                   "use RolloutCollector(..., value_input='privileged') with value_fn=FusedMlpValue(MlpValue(52), ...) or a torch value_fn"),
    ("goal", "goal observations (its policy kernels read the 13-column observation); "
             "use RolloutCollector(..., policy_input='observation+goal') with FusedMlpPolicy(MlpActorCritic(obs_dim=21), ...) "
             "or a torch policy"),
    ("track_ids", "a track bank (its sampling-fused step kernels fly the one track of the env); "
                  "use RolloutCollector with a torch policy"),
    ("history", "history rows (its policy kernels read the 13-column observation); "
                "use RolloutCollector(..., policy_input='history') with FusedMlpPolicy(MlpActorCritic(obs_dim=W), ...) or a torch policy"))


def _refuse_extra_rows(env, who):
    for attr, what in _EXTRA_ROWS:
        if getattr(env, attr, None) is not None:
            raise ValueError(f"{who} does not carry {what}")


def _sampling_fused_scope(env):
    """Whether the sampling-fused step kernels (dn_step_sampled, dn_step_squashed) are built for this env: no reward wrappers, extra
    physics terms, RPM / PID actions, random spawn or per-drone models.  Outside it a collector samples and steps in two launches."""
    cfg = env.cfg
    return not (cfg.clip_rew or cfg.norm_rew or cfg.physics or cfg.action_type or cfg.random_spawn or cfg.zero_damping
                or env.dynamics is not None or env.wind is not None or env.actuator is not None or env.sensor is not None)


class RolloutCollector:
    """n_steps x (policy -> dn_step) on one GPU's shard, then GAE (+ optional all-gather).

    policy(obs[N,13] f32) -> (actions[N,4] f32, values[N] f32, log_probs[N] f32), all on the env's device;
    value_fn(obs) -> values[N] (defaults to the policy's second output).  Actions are clipped to the action
    space before the step, as SB3 does.  `bootstrap_truncated` adds gamma * V(terminal_observation) to the reward
    of drones whose episode hit the time limit (SB3's TimeLimit handling).

    `use_graph`: the whole rollout -- n_steps x (policy kernels, clip, dn_step, bootstrap, buffer writes) and the
    GAE kernel -- is captured into one hipGraph on the second call to collect() (the first call runs eagerly and
    doubles as the warm-up) and replayed afterwards: the loop is launch-bound (a 13->512->512->256 MLP step is a
    dozen small kernels), and a graph replay takes the host out of it.  Every tensor the loop touches is a static
    buffer; the environment's vector-step counter lives on the device, so noise streams keep advancing under replay.
    The policy must be capture-safe (no host synchronisation, no data-dependent shapes).

    `value_input="privileged"` (asymmetric actor-critic; the env needs privileged=PrivilegedObservation(...), and `value_fn` is
    required): the critic sees the env's privileged rows [N, 52] instead of the observation -- `values[t]` is value_fn of the rows that
    go with `obs[t]`, the truncation bootstrap is value_fn of the TERMINAL privileged rows (the true terminal state with the finished
    episode's parameters, where the terminal observation is the delayed and biased one), `last_values` is value_fn of the last rows,
    and the buffer dict gains `privileged` [n_steps, N, 52].  The policy's own value output is ignored.

    `policy_input="observation+goal"` (the env needs goal=GoalObservation(...)): the policy -- and the value function, unless
    `value_input="privileged"` -- sees cat(obs, goal), [N, obs_dim + 8]; the truncation bootstrap is evaluated on
    cat(terminal_obs, terminal_goal), and the buffer dict gains `goal` [n_steps, N, 8] (`obs` stays the observation alone).

    `policy_input="history"` (the env needs history=HistoryObservation(...)): the policy -- and the value function, unless
    `value_input="privileged"` -- sees `env.history`, [N, W]; the truncation bootstrap is evaluated on `terminal_history` where done, and
    the buffer dict gains `history` [n_steps, N, W] (`obs` stays the 13 columns).

    An env with a track bank (tracks=TrackBank(...)): the buffer dict gains `track` [n_steps, N] int32, the track each drone is on
    when `obs[t]` is observed.

    `policy_norm=RowNormalizer(W, device)`: what the policy is shown -- `obs`, cat(obs, goal) or the history rows, and the value function
    too when it reads observations -- passes through a fleet-wide running normaliser (rownorm.py), in SB3's VecNormalize order [from
    recall]: the reset rows and, after each step, the next rows update the statistics and are normalised with the updated ones; the rows
    of the truncation bootstrap, where(done, terminal, next), are normalised with the same statistics and do not move them.  The buffer
    dict gains `policy_rows` [n_steps, N, W], the rows the policy saw -- what a learner trains on; `obs`, `goal` and `history` stay raw.
    `value_norm=RowNormalizer(52, device)` (needs value_input="privileged"): the same three rules for the privileged rows, and the buffer
    dict gains `value_rows` [n_steps, N, 52].  A width that does not match the rows is a ValueError.  Both work under `use_graph`: the
    statistics live on the device and keep moving under replay.  Each rank keeps its own statistics.

    `reward_norm=ReturnNormalizer(N, device)` (retnorm.py): the reward half of VecNormalize [from recall].  After the step the raw reward
    goes to the new buffer key `raw_rewards` [n_steps, N]; the reward is scaled with `update_normalize(reward, next_done)` (the fleet's
    discounted returns update one RunningMeanStd, the reward is divided by their standard deviation and clipped); THEN the truncation
    bootstrap gamma * V(terminal) * truncated is added, SB3's order: VecNormalize sits inside the algorithm's TimeLimit handling, so the
    critic lives in the normalised scale.  `rewards` is what GAE reads.  The normaliser's gamma is its own, not the collector's.  A
    normaliser of another num_envs or device is a ValueError.  Works under `use_graph`.  The Monitor episode returns stay raw."""

    def __init__(self, env, policy, n_steps, *, value_fn=None, gamma=0.99, gae_lambda=0.95, bootstrap_truncated=True,
                 gather=False, group=None, use_graph=False, value_input="observation", policy_input="observation",
                 policy_norm=None, value_norm=None, reward_norm=None):
        from .vec_env import ACT_DIM, DroneVecEnv
        if policy_input not in ("observation", "observation+goal", "history"):       # a misspelt mode is wrong whatever the env
            raise ValueError(f"policy_input must be 'observation', 'observation+goal' or 'history', got {policy_input!r}")
        if value_norm is not None and value_input != "privileged":
            raise ValueError("value_norm needs value_input='privileged' (a value function on observations sees the policy's rows: "
                             "use policy_norm)")
        if policy_norm is not None or value_norm is not None:
            from .rownorm import RowNormalizer
            for name, v in (("policy_norm", policy_norm), ("value_norm", value_norm)):
                if v is not None and not isinstance(v, RowNormalizer):
                    raise TypeError(f"{name} must be a RowNormalizer or None, got {type(v).__name__}")
            if policy_norm is value_norm:
                raise ValueError("policy_norm and value_norm must be two normalisers: each keeps the statistics of one kind of row")
        if reward_norm is not None:
            from .retnorm import ReturnNormalizer
            if not isinstance(reward_norm, ReturnNormalizer):
                raise TypeError(f"reward_norm must be a ReturnNormalizer or None, got {type(reward_norm).__name__}")
        if not isinstance(env, DroneVecEnv):
            raise TypeError("RolloutCollector drives a DroneVecEnv (HIP); there is no CPU path")
        if reward_norm is not None and (reward_norm.num_envs != env.num_envs or reward_norm.device != env.device):
            raise ValueError(f"reward_norm is of {reward_norm.num_envs} envs on {reward_norm.device}; the env has {env.num_envs} on "
                             f"{env.device}")
        if value_input not in ("observation", "privileged"):
            raise ValueError(f"value_input must be 'observation' or 'privileged', got {value_input!r}")
        self.value_privileged = value_input == "privileged"
        if self.value_privileged:
            if env.privileged is None:
                raise ValueError("value_input='privileged' needs an env built with privileged=PrivilegedObservation(...)")
            if value_fn is None:
                raise ValueError("value_input='privileged' needs value_fn: the policy's own value head sees the observation")
        self.policy_goal = policy_input == "observation+goal"
        if self.policy_goal and env.goal is None:
            raise ValueError("policy_input='observation+goal' needs an env built with goal=GoalObservation(...)")
        self.policy_history = policy_input == "history"
        if self.policy_history and env.history is None:
            raise ValueError("policy_input='history' needs an env built with history=HistoryObservation(...)")
        self.env, self.policy, self.value_fn = env, policy, value_fn
        self.n_steps, self.gamma, self.gae_lambda = int(n_steps), float(gamma), float(gae_lambda)
        self.bootstrap_truncated, self.gather, self.group = bool(bootstrap_truncated), bool(gather), group
        self.use_graph = bool(use_graph)
        import inspect
        try:        # a value function that can skip unflagged tiles (FusedMlpPolicy.predict_values) gets the truncation mask
            self._value_fn_takes_mask = value_fn is not None and "row_mask" in inspect.signature(value_fn).parameters
        except (TypeError, ValueError):
            self._value_fn_takes_mask = False
        n, T, dev, f32 = env.num_envs, self.n_steps, env.device, torch.float32
        self.buf = dict(
            obs=torch.empty((T, n, env.obs_dim), dtype=f32, device=dev),
            actions=torch.empty((T, n, ACT_DIM), dtype=f32, device=dev),
            values=torch.empty((T, n), dtype=f32, device=dev), log_probs=torch.empty((T, n), dtype=f32, device=dev),
            rewards=torch.empty((T, n), dtype=f32, device=dev),
            episode_starts=torch.empty((T, n), dtype=torch.uint8, device=dev),
            advantages=torch.empty((T, n), dtype=f32, device=dev), returns=torch.empty((T, n), dtype=f32, device=dev),
            last_values=torch.empty(n, dtype=f32, device=dev), last_dones=torch.empty(n, dtype=torch.uint8, device=dev))
        self._clipped = torch.empty((n, ACT_DIM), dtype=f32, device=dev)
        self._last_obs = env.reset_tensor().clone()
        # the rows carried beside the observation, by the key they have in `info` and in the buffer dict: a static tensor each, which
        # holds what goes with `_last_obs` (the track: the one each drone is on when obs[t] is observed)
        self._last = {}
        for wanted, key, rows in ((self.value_privileged, "privileged", env.privileged), (self.policy_goal, "goal", env.goal),
                                  (self.policy_history, "history", env.history), (env.track_ids is not None, "track", env.track_ids)):
            if wanted:
                self.buf[key] = torch.empty((T,) + tuple(rows.shape), dtype=rows.dtype, device=dev)
                self._last[key] = rows.clone()
        self._last_done = torch.ones(n, dtype=torch.uint8, device=dev)       # SB3: _last_episode_starts = True
        self.policy_norm, self.value_norm = policy_norm, value_norm
        for name, norm, rows in (("policy_norm", policy_norm, self._seen(self._last_obs, self._last)),
                                 ("value_norm", value_norm, self._last.get("privileged"))):
            if norm is None:
                continue
            if norm.width != rows.shape[1] or norm.device != dev:
                raise ValueError(f"{name} is of width {norm.width} on {norm.device}; the rows it is to normalise are "
                                 f"{rows.shape[1]} columns wide on {dev}")
            key = "policy_rows" if norm is policy_norm else "value_rows"
            self.buf[key] = torch.empty((T, n, norm.width), dtype=f32, device=dev)
            setattr(self, "_" + key, norm.update_normalize(rows))          # the reset rows: VecNormalize.reset updates, then normalises
        self.reward_norm = reward_norm
        if reward_norm is not None:
            self.buf["raw_rewards"] = torch.empty((T, n), dtype=f32, device=dev)
            self._norm_reward = torch.empty(n, dtype=f32, device=dev)
        self.num_timesteps = 0
        self._graph = None
        self._calls = 0

    def _seen(self, o, rows, terminal=""):
        """The raw rows the policy (and the value function on observations) is shown: `rows` maps the carried keys to the rows that go
        with observation `o` -- the collector's own, or a step's `info`, whose terminal rows are the keys behind "terminal_"."""
        if self.policy_history:
            return rows[terminal + "history"]
        return torch.cat((o, rows[terminal + "goal"]), dim=1) if self.policy_goal else o

    def _values(self, obs, row_mask=None):
        if self.value_fn is not None:
            if row_mask is not None and self._value_fn_takes_mask:
                return self.value_fn(obs, row_mask=row_mask).reshape(-1)
            return self.value_fn(obs).reshape(-1)
        return self.policy(obs)[1].reshape(-1)

    def _rollout(self):
        """One rollout on the current stream, in place in the static buffers (eager or under graph capture)."""
        from . import _capi
        import ctypes as C
        env, b, last = self.env, self.buf, self._last
        obs, done = self._last_obs, self._last_done
        priv = last.get("privileged")
        seen = self._seen
        # with a normaliser the policy / the critic read its static buffer, the normalised image of the current raw rows
        pn, vn = self.policy_norm, self.value_norm

        for t in range(self.n_steps):
            actions, values, log_probs = self.policy(seen(obs, last) if pn is None else self._policy_rows)
            if pn is not None:
                b["policy_rows"][t].copy_(self._policy_rows)
            for key, rows in last.items():
                b[key][t].copy_(rows)
            if priv is not None:
                if vn is not None:
                    b["value_rows"][t].copy_(self._value_rows)
                values = self._values(priv if vn is None else self._value_rows)
            b["obs"][t].copy_(obs)
            b["episode_starts"][t].copy_(done)
            b["values"][t].copy_(values.reshape(-1))
            b["log_probs"][t].copy_(log_probs.reshape(-1))
            b["actions"][t].copy_(actions)
            torch.clamp(b["actions"][t], -1.0, 1.0, out=self._clipped)
            next_obs, reward, next_done, info = env.step_tensor(self._clipped, want_terminal=self.bootstrap_truncated)
            # VecNormalize.step_wait: the next rows update the statistics and are normalised; the terminal rows below see the same statistics
            if pn is not None:
                pn.update_normalize(seen(next_obs, info), out=self._policy_rows)
            if vn is not None:
                vn.update_normalize(info["privileged"], out=self._value_rows)
            if self.reward_norm is not None:    # before the bootstrap below: the critic's values are in the normalised scale already
                b["raw_rewards"][t].copy_(reward)
                reward = self.reward_norm.update_normalize(reward, next_done, out=self._norm_reward)
            if self.bootstrap_truncated:
                # rows of terminal_obs are valid only where done; `truncated` is zero elsewhere
                if priv is not None:
                    rows = torch.where(next_done.bool()[:, None], info["terminal_privileged"], info["privileged"])
                    tv = self._values(rows if vn is None else vn.normalize(rows, out=rows), row_mask=info["truncated"])
                else:
                    rows = torch.where(next_done.bool()[:, None], seen(info["terminal_obs"], info, "terminal_"), seen(next_obs, info))
                    tv = self._values(rows if pn is None else pn.normalize(rows, out=rows), row_mask=info["truncated"])
                reward = reward + self.gamma * tv * info["truncated"].to(reward.dtype)
            b["rewards"][t].copy_(reward)
            obs.copy_(next_obs)
            done.copy_(next_done)
            for key, rows in last.items():
                rows.copy_(info[key])
        if priv is not None:
            b["last_values"].copy_(self._values(priv if vn is None else self._value_rows))
        else:
            b["last_values"].copy_(self._values(seen(obs, last) if pn is None else self._policy_rows))
        b["last_dones"].copy_(done)
        dev = env.device
        _capi.check(_capi.load().dn_gae(
            b["rewards"].data_ptr(), b["values"].data_ptr(), b["episode_starts"].data_ptr(), b["last_values"].data_ptr(),
            b["last_dones"].data_ptr(), self.n_steps, env.num_envs, self.gamma, self.gae_lambda,
            b["advantages"].data_ptr(), b["returns"].data_ptr(), dev.index,
            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))

    @torch.no_grad()
    def collect(self):
        """One rollout.  Returns the buffer dict (static tensors, overwritten by the next call) with `advantages`,
        `returns` ([n_steps, N_local]) and, with `gather`, `advantages_global` / `returns_global` ([n_steps, N_global])."""
        env = self.env
        with torch.cuda.device(env.device):
            if self.use_graph and self._calls >= 1:
                if self._graph is None:
                    torch.cuda.synchronize(env.device)
                    self._graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self._graph):
                        self._rollout()
                self._graph.replay()
            else:
                self._rollout()
        self._calls += 1
        self.num_timesteps += self.n_steps * env.num_envs
        out = dict(self.buf)
        if self.gather:
            out["advantages_global"], out["returns_global"] = all_gather_rollout(out["advantages"], out["returns"], self.group)
        return out


class ReplayBuffer:
    """Device-resident ring buffer with the layout and semantics of SB3's `ReplayBuffer` as the reference's SAC/DDPG
    agents use it (PBDroneSimulator.py:297-338; `SaveReplayBufferCallback`, Sol/Utilities/Callbacks.py:13-39)
    [3P-recall]: per slot and drone `obs`, `next_obs` (the TERMINAL observation where the episode ended, not the reset
    one), `action`, `reward`, `done` (with `handle_timeout_termination`: a TimeLimit truncation is stored as not done)
    and `timeout`.  Step-major [buffer_size, N, ...]; `add` is a handful of in-place copies, `sample` a gather."""

    def __init__(self, buffer_size, num_envs, obs_dim, act_dim, device):
        f32, dev = torch.float32, torch.device(device)
        self.buffer_size, self.num_envs = int(buffer_size), int(num_envs)
        self.obs = torch.empty((self.buffer_size, num_envs, obs_dim), dtype=f32, device=dev)
        self.next_obs = torch.empty_like(self.obs)
        self.actions = torch.empty((self.buffer_size, num_envs, act_dim), dtype=f32, device=dev)
        self.rewards = torch.empty((self.buffer_size, num_envs), dtype=f32, device=dev)
        self.dones = torch.empty((self.buffer_size, num_envs), dtype=f32, device=dev)
        self.timeouts = torch.empty((self.buffer_size, num_envs), dtype=f32, device=dev)
        self.pos, self.full = 0, False

    def add(self, obs, next_obs, action, reward, done, timeout):
        p = self.pos
        self.obs[p].copy_(obs)
        self.next_obs[p].copy_(next_obs)
        self.actions[p].copy_(action)
        self.rewards[p].copy_(reward)
        self.dones[p].copy_(done)
        self.timeouts[p].copy_(timeout)
        self.pos = (p + 1) % self.buffer_size
        self.full = self.full or self.pos == 0

    def __len__(self):
        return (self.buffer_size if self.full else self.pos) * self.num_envs

    def sample(self, batch_size, generator=None):
        upper = self.buffer_size if self.full else self.pos
        if upper == 0:
            raise RuntimeError("the replay buffer is empty")
        dev = self.obs.device
        t = torch.randint(0, upper, (batch_size,), device=dev, generator=generator)
        e = torch.randint(0, self.num_envs, (batch_size,), device=dev, generator=generator)
        return dict(obs=self.obs[t, e], next_obs=self.next_obs[t, e], actions=self.actions[t, e], rewards=self.rewards[t, e],
                    dones=self.dones[t, e] * (1.0 - self.timeouts[t, e]))


class RingReplayBuffer:
    """The same transitions as ReplayBuffer, laid out so that the kernels write them in place: `obs_ring[t + 1]` is both the
    observation the step at slot t produced and the input of the step at slot t + 1 (SB3's `optimize_memory_usage` idea, with one
    spare row, so that every slot is whole at a cycle boundary; mid-cycle the slot being replaced is excluded), `terminal_obs[t]` holds the terminal observations dn_step reports, `dones` /
    `timeouts` stay the uint8 flags the kernel writes.  SB3's view of a transition is assembled on demand: `next_obs` = the
    TERMINAL observation where the episode ended, the next one elsewhere; `dones`, `timeouts` as float32."""

    def __init__(self, buffer_size, num_envs, obs_dim, act_dim, device):
        f32, u8, dev = torch.float32, torch.uint8, torch.device(device)
        self.buffer_size, self.num_envs = int(buffer_size), int(num_envs)
        self.obs_ring = torch.zeros((self.buffer_size + 1, num_envs, obs_dim), dtype=f32, device=dev)
        self.terminal_obs = torch.zeros((self.buffer_size, num_envs, obs_dim), dtype=f32, device=dev)
        self.actions = torch.zeros((self.buffer_size, num_envs, act_dim), dtype=f32, device=dev)
        self.rewards = torch.zeros((self.buffer_size, num_envs), dtype=f32, device=dev)
        self.done_flags = torch.zeros((self.buffer_size, num_envs), dtype=u8, device=dev)
        self.timeout_flags = torch.zeros((self.buffer_size, num_envs), dtype=u8, device=dev)
        self.pos, self.full = 0, False

    obs = property(lambda self: self.obs_ring[:self.buffer_size])
    next_obs = property(lambda self: torch.where(self.done_flags.bool()[..., None], self.terminal_obs, self.obs_ring[1:]))
    dones = property(lambda self: self.done_flags.float())
    timeouts = property(lambda self: self.timeout_flags.float())

    def valid_slots(self):
        """Slots whose transition is whole.  Mid-cycle on a full ring the OLDEST slot (= pos, the next to be written) has lost
        its observation to the newest transition's next observation (they share a row); at a cycle boundary (pos = 0) the
        spare row keeps all buffer_size slots whole."""
        if not self.full:
            return list(range(self.pos))
        return [t for t in range(self.buffer_size) if t != self.pos or self.pos == 0]

    def __len__(self):
        return len(self.valid_slots()) * self.num_envs

    def _sample_slots(self, batch_size, generator=None):
        dev = self.obs_ring.device
        upper = (self.buffer_size - (1 if self.pos else 0)) if self.full else self.pos
        if upper == 0:
            raise RuntimeError("the replay buffer is empty")
        t = torch.randint(0, upper, (batch_size,), device=dev, generator=generator)
        if self.full and self.pos:
            t = t + (t >= self.pos).long()                                   # skip the slot that is being replaced
        return t, torch.randint(0, self.num_envs, (batch_size,), device=dev, generator=generator)

    def sample(self, batch_size, generator=None):
        t, e = self._sample_slots(batch_size, generator)
        d = self.done_flags[t, e].bool()
        return dict(obs=self.obs_ring[t, e], next_obs=torch.where(d[:, None], self.terminal_obs[t, e], self.obs_ring[t + 1, e]),
                    actions=self.actions[t, e], rewards=self.rewards[t, e],
                    dones=d.float() * (1.0 - self.timeout_flags[t, e].float()))


class OffPolicyCollector:
    """BASELINE config 5's collection loop (SAC: one environment step per policy step, every transition into the
    replay buffer): actor(obs) -> actions in [-1, 1] -> dn_step -> replay buffer, with SB3's terminal-observation
    handling.  Sharded like the on-policy collector: a rank's drones feed the rank's buffer, no collective.

    With a policy_mfma.FusedSacActor the loop is two launches per step and no copies: dn_mlp_forward (mu | log_std from the
    ring's current observation row) and dn_step_squashed (clamp, Philox draw, tanh inside the step kernel: the action, the next
    observation, reward, flags and terminal observation land in their buffer slots) -- RingReplayBuffer; three launches
    (dn_squashed_sample + dn_step, the same bits) with `fused_sample=False` or with the options dn_step_squashed is not built for.  With any other
    torch callable the actions come from the callable and the transitions are copied into a ReplayBuffer.

    `collect_cycle()`: one whole pass over the ring buffer (buffer_size steps, slot 0 .. buffer_size - 1) captured into
    a hipGraph on its second call and replayed afterwards -- every tensor of the loop is static and the ring position is
    back where it started, so the host leaves the loop as it does for RolloutCollector(use_graph=True)."""

    def __init__(self, env, actor, buffer_size, *, seed=0, deterministic=False, fused_sample=True):
        from .policy_mfma import FusedSacActor
        from .vec_env import ACT_DIM, DroneVecEnv
        _refuse_extra_rows(env, "OffPolicyCollector")
        if not isinstance(env, DroneVecEnv):
            raise TypeError("OffPolicyCollector drives a DroneVecEnv (HIP); there is no CPU path")
        self.env, self.actor = env, actor
        self.direct = isinstance(actor, FusedSacActor)
        self.seed, self.deterministic = int(seed), bool(deterministic)
        if self.direct:
            if env.obs_dim != 13 or env.num_envs != actor._out.shape[0]:
                raise ValueError("the direct loop needs the full 13-column observation and an actor built for env.num_envs drones")
            self.buffer = RingReplayBuffer(buffer_size, env.num_envs, env.obs_dim, ACT_DIM, env.device)
            self.buffer.obs_ring[0].copy_(env.reset_tensor())
            self._found = torch.zeros(env.num_envs, dtype=torch.int32, device=env.device)
            self._fused_sample = fused_sample and _sampling_fused_scope(env)      # dn_step_squashed's scope
        else:
            self.buffer = ReplayBuffer(buffer_size, env.num_envs, env.obs_dim, ACT_DIM, env.device)
            self._obs = env.reset_tensor().clone()
        self.num_timesteps = 0
        self._graph, self._cycles, self._carry = None, 0, False

    def _steps_direct(self, n_steps):
        import ctypes as C
        from . import _capi
        from .policy_mfma import mlp_forward
        env, buf, lib = self.env, self.buffer, _capi.load()
        h, T = env._handle, buf.buffer_size
        sptr = C.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
        out8 = self.actor._out
        for _ in range(int(n_steps)):
            p = buf.pos
            if p == 0 and self._carry:                      # wrapped: the newest observation (row T) becomes row 0 only now, when
                buf.obs_ring[0].copy_(buf.obs_ring[T])      # slot 0's old transition is about to be replaced as a whole
                self._carry = False
            mlp_forward([self.actor.pack], buf.obs_ring[p], [out8])
            outs = (buf.obs_ring[p + 1].data_ptr(), buf.rewards[p].data_ptr(), buf.done_flags[p].data_ptr(), buf.timeout_flags[p].data_ptr(),
                    self._found.data_ptr(), buf.terminal_obs[p].data_ptr(), None, None, None, sptr)
            if self._fused_sample:                          # the draw inside the step kernel: two launches per step
                _capi.check(lib.dn_step_squashed(h, out8.data_ptr(), self.seed, int(self.deterministic), buf.actions[p].data_ptr(), None, *outs))
            else:
                _capi.check(lib.dn_squashed_sample(h, out8.data_ptr(), self.seed, int(self.deterministic), buf.actions[p].data_ptr(), None, sptr))
                _capi.check(lib.dn_step(h, buf.actions[p].data_ptr(), *outs))
            buf.pos = p + 1
            if buf.pos == T:
                buf.pos, buf.full, self._carry = 0, True, True

    def _steps(self, n_steps):
        if self.direct:
            return self._steps_direct(n_steps)
        env = self.env
        for _ in range(int(n_steps)):
            actions = self.actor(self._obs).clamp(-1.0, 1.0)
            next_obs, reward, done, info = env.step_tensor(actions, want_terminal=True)
            d = done.bool()[:, None]
            self.buffer.add(self._obs, torch.where(d, info["terminal_obs"], next_obs), actions, reward, done.float(),
                            info["truncated"].float())
            self._obs.copy_(next_obs)

    @torch.no_grad()
    def collect(self, n_steps=1):
        with torch.cuda.device(self.env.device):
            self._steps(n_steps)
        self.num_timesteps += int(n_steps) * self.env.num_envs
        return self.buffer

    @torch.no_grad()
    def collect_cycle(self):
        if self.buffer.pos != 0:
            raise RuntimeError("collect_cycle() fills slots 0 .. buffer_size - 1: call it with the ring at position 0")
        T = self.buffer.buffer_size
        with torch.cuda.device(self.env.device):
            if self._cycles >= 1:
                if self._graph is None:
                    torch.cuda.synchronize(self.env.device)
                    self._graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self._graph):
                        self._steps(T)
                    self.buffer.pos = 0                     # the capture pass advanced the host-side ring position only
                self._graph.replay()
                self.buffer.full, self._carry = True, True
            else:
                self._steps(T)
        self._cycles += 1
        self.num_timesteps += T * self.env.num_envs
        return self.buffer


class FusedRolloutCollector:
    """The on-policy rollout with every per-step operation on a purpose-built kernel and no intermediate copies:

        dn_mlp_forward (actor + critic, one launch; the value lands in the rollout buffer)
        dn_step_sampled (Gaussian sample from the environment's Philox streams, clip, log-probability -> buffer, and the
                         step itself: next observation, reward and episode-start flag straight into the buffer slots)
    two launches per step instead of ~25 small torch kernels -- or ONE with `one_launch=True` (dn_mlp_step_sampled: the policy kernel's
    workgroups step the drones they evaluated; the same bits).  Off by default because it measured SLOWER on MI355X at 32 768 drones
    (80.7 against 69.9 us per step with bf16 networks, 179.9 against 174.1 in the float32 grade): the single step is latency bound, inside
    the policy kernel it runs on the critical path of every actor workgroup with nothing to overlap it (LDS keeps one workgroup per CU),
    and the step's registers push spills into the MFMA loops; the kernel boundary it removes costs 1.7 us (profiles/r03_notes.md); then, once per rollout, SB3's TimeLimit bootstrap
    (rewards[t] += gamma V(terminal_observation) where TimeLimit.truncated): the step kernel leaves the terminal
    observations and truncation flags of all n_steps in the buffer, ONE dn_mlp_forward masked by those flags evaluates
    the critic on the tiles that hold a truncated drone (the weights do not change inside a rollout, so this is the
    value SB3 computes on the spot) and ONE dn_add_bootstrap adds it; then dn_gae.  The whole rollout is captured into one
    hipGraph on the second call (`use_graph`).  Same results contract as RolloutCollector (SB3 collect_rollouts
    semantics); the action noise comes from Philox (seed, global drone id, step counter), so a rollout is reproducible
    and independent of how the drones are sharded.  Call `policy.refresh()` after optimiser steps (it re-packs in place, so
    the captured launches see the new weights); a changed log_std (baked into the captured launches by value) is noticed at the
    next collect(), which captures again (`recapture()` forces it).
    With `gather`, `advantages_global` / `returns_global` are [n_steps, R, N_local] views of a static receive buffer
    (RolloutGather: one all_gather_into_tensor per rollout, nothing allocated or copied per rollout)."""

    def __init__(self, env, policy, n_steps, *, gamma=0.99, gae_lambda=0.95, bootstrap_truncated=True, gather=False,
                 group=None, use_graph=True, seed=0, one_launch=False):
        from .policy_mfma import FusedMlpPolicy
        from .vec_env import ACT_DIM, OBS_DIM, DroneVecEnv
        _refuse_extra_rows(env, "FusedRolloutCollector")
        if not isinstance(env, DroneVecEnv) or not isinstance(policy, FusedMlpPolicy):
            raise TypeError("FusedRolloutCollector needs a DroneVecEnv and a FusedMlpPolicy (HIP); there is no CPU path")
        if env.num_envs % 4 or env.obs_dim != OBS_DIM:
            raise ValueError("num_envs must be a multiple of 4 and the observation the full 13 columns")
        if policy.pi["obs_dim"] != OBS_DIM or policy.vf["obs_dim"] != OBS_DIM:      # dn_mlp_step_sampled takes the pointers without the widths
            raise ValueError(f"FusedRolloutCollector feeds its policy the {OBS_DIM}-column observation; the policy was packed for "
                             f"{policy.pi['obs_dim']} (actor) / {policy.vf['obs_dim']} (critic) columns")
        self.env, self.policy = env, policy
        self.n_steps, self.gamma, self.gae_lambda = int(n_steps), float(gamma), float(gae_lambda)
        self.bootstrap_truncated, self.gather, self.group, self.use_graph = bool(bootstrap_truncated), bool(gather), group, bool(use_graph)
        self.seed = int(seed)
        n, T, dev, f32, u8 = env.num_envs, self.n_steps, env.device, torch.float32, torch.uint8
        self.buf = dict(
            obs=torch.empty((T + 1, n, OBS_DIM), dtype=f32, device=dev),
            actions=torch.empty((T, n, ACT_DIM), dtype=f32, device=dev),
            values=torch.empty((T, n), dtype=f32, device=dev), log_probs=torch.empty((T, n), dtype=f32, device=dev),
            rewards=torch.empty((T, n), dtype=f32, device=dev),
            episode_starts=torch.ones((T + 1, n), dtype=u8, device=dev),          # SB3: _last_episode_starts = True
            last_values=torch.empty((n, 1), dtype=f32, device=dev))
        # advantages / returns live in the all-gather's send buffer (RolloutGather): dn_gae writes them where RCCL reads them
        self._gather = RolloutGather(T, n, dev, group) if self.gather else None
        if self._gather is not None:
            self.buf["advantages"], self.buf["returns"] = self._gather.advantages, self._gather.returns
        else:
            self.buf["advantages"], self.buf["returns"] = torch.empty((T, n), dtype=f32, device=dev), torch.empty((T, n), dtype=f32, device=dev)
        self._mean = torch.empty((n, ACT_DIM), dtype=f32, device=dev)
        cfg = env.cfg
        self._sampled_step = _sampling_fused_scope(env)       # dn_step_sampled's scope (outside it: sample + dn_step)
        self._clipped = None if self._sampled_step else torch.empty((n, ACT_DIM), dtype=f32, device=dev)
        # ONE launch per step (dn_mlp_step_sampled: the actor's workgroups step the drones they evaluated) where that kernel is built:
        # the float64 reference configuration without noise / ground contact, fleets on the three-wave single step, whole workgroups
        self._one_launch = bool(one_launch) and self._sampled_step and not (cfg.ground_contact or cfg.act_noise_sigma > 0 or cfg.obs_noise_sigma > 0
                                                                          or cfg.compute_f32) \
            and env.kernel_waves(fused=False) == 3 and n % (64 if policy.grade == "fp32" else 128) == 0
        self._trunc = torch.zeros((T, n), dtype=u8, device=dev)
        self._found = torch.zeros(n, dtype=torch.int32, device=dev)
        # terminal observations of every step of the rollout (rows are written where a drone finished; the rest is stale
        # and never used: the masked forward and the bootstrap select by `truncated`)
        self._term_obs = torch.zeros((T, n, OBS_DIM), dtype=f32, device=dev) if self.bootstrap_truncated else None
        self._tv = torch.zeros((T * n, 1), dtype=f32, device=dev)
        self.buf["obs"][0].copy_(env.reset_tensor())
        self.num_timesteps = 0
        self._graph, self._calls, self._captured_log_std = None, 0, None

    def recapture(self):
        self._graph = None

    def _rollout(self):
        import ctypes as C
        from . import _capi
        from .policy_mfma import mlp_forward
        env, pol, b, T = self.env, self.policy, self.buf, self.n_steps
        lib, h, n, dev = _capi.load(), env._handle, env.num_envs, env.device
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        log_std = (C.c_float * 4)(*[float(x) for x in pol.log_std_host])
        from .policy_mfma import _net_struct
        for t in range(T):
            obs_t = b["obs"][t]
            term = self._term_obs[t].data_ptr() if self.bootstrap_truncated else None
            if self._one_launch:
                # policy forward (actor + critic), Gaussian sample, clip, log-probability and the environment step in ONE launch
                nets = (_capi.DnMlpNet * 2)(_net_struct(pol.pi, self._mean), _net_struct(pol.vf, b["values"][t].view(n, 1)))
                _capi.check(lib.dn_mlp_step_sampled(h, C.cast(nets, C.c_void_p), 2, obs_t.data_ptr(), obs_t.shape[1], log_std, self.seed, 0,
                                                    b["actions"][t].data_ptr(), b["log_probs"][t].data_ptr(), b["obs"][t + 1].data_ptr(),
                                                    b["rewards"][t].data_ptr(), b["episode_starts"][t + 1].data_ptr(), self._trunc[t].data_ptr(),
                                                    self._found.data_ptr(), term, None, None, None, stream))
                continue
            mlp_forward([pol.pi, pol.vf], obs_t, [self._mean, b["values"][t].view(n, 1)])
            if self._sampled_step:
                # Gaussian sample (Philox), clip, log-probability and the environment step in ONE launch (dn_step_sampled)
                _capi.check(lib.dn_step_sampled(h, self._mean.data_ptr(), log_std, self.seed, 0, b["actions"][t].data_ptr(),
                                                b["log_probs"][t].data_ptr(), b["obs"][t + 1].data_ptr(), b["rewards"][t].data_ptr(),
                                                b["episode_starts"][t + 1].data_ptr(), self._trunc[t].data_ptr(),
                                                self._found.data_ptr(), term, None, None, None, stream))
            else:                                              # reward wrappers / extra physics terms / RPM actions: two launches
                _capi.check(lib.dn_policy_sample(h, self._mean.data_ptr(), log_std, self.seed, 0, b["actions"][t].data_ptr(),
                                                 self._clipped.data_ptr(), b["log_probs"][t].data_ptr(), stream))
                _capi.check(lib.dn_step(h, self._clipped.data_ptr(), b["obs"][t + 1].data_ptr(), b["rewards"][t].data_ptr(),
                                        b["episode_starts"][t + 1].data_ptr(), self._trunc[t].data_ptr(), self._found.data_ptr(),
                                        term, None, None, None, stream))
        if self.bootstrap_truncated:
            mlp_forward([pol.vf], self._term_obs.view(T * n, -1), [self._tv], row_mask=self._trunc.view(T * n))
            _capi.check(lib.dn_add_bootstrap(b["rewards"].data_ptr(), self._tv.data_ptr(), self._trunc.data_ptr(),
                                             self.gamma, T * n, dev.index, stream))
        mlp_forward([pol.vf], b["obs"][T], [b["last_values"]])
        _capi.check(lib.dn_gae(b["rewards"].data_ptr(), b["values"].data_ptr(), b["episode_starts"].data_ptr(),
                               b["last_values"].data_ptr(), b["episode_starts"][T].data_ptr(), T, n, self.gamma,
                               self.gae_lambda, b["advantages"].data_ptr(), b["returns"].data_ptr(), dev.index, stream))

    @torch.no_grad()
    def collect(self):
        """One rollout; returns views of the static buffers (obs / episode_starts hold n_steps + 1 slots: the last one is
        the observation / start flag the next rollout begins with)."""
        env, b, T = self.env, self.buf, self.n_steps
        with torch.cuda.device(env.device):
            if self._calls > 0:                            # carry the last observation / start flags over
                b["obs"][0].copy_(b["obs"][T])
                b["episode_starts"][0].copy_(b["episode_starts"][T])
            if self.use_graph and self._calls >= 1:
                # dn_step_sampled takes log_std by value (a HOST float[4]): it is baked into the captured launches, so a
                # refresh() that moved it (PPO trains log_std) makes the graph stale -- capture again
                if self._graph is not None and tuple(self.policy.log_std_host) != self._captured_log_std:
                    self._graph = None
                if self._graph is None:
                    torch.cuda.synchronize(env.device)
                    self._graph = torch.cuda.CUDAGraph()
                    self._captured_log_std = tuple(self.policy.log_std_host)
                    with torch.cuda.graph(self._graph):
                        self._rollout()
                self._graph.replay()
            else:
                self._rollout()
        self._calls += 1
        self.num_timesteps += T * env.num_envs
        out = dict(obs=b["obs"][:T], actions=b["actions"], values=b["values"], log_probs=b["log_probs"], rewards=b["rewards"],
                   episode_starts=b["episode_starts"][:T], advantages=b["advantages"], returns=b["returns"],
                   last_values=b["last_values"].view(-1), last_dones=b["episode_starts"][T], next_obs=b["obs"][T])
        if self.gather:
            # [n_steps, R, N_local] strided views of the static receive buffer ([t, r, i] = global drone r * N_local + i)
            out["advantages_global"], out["returns_global"] = self._gather.gather()
        return out
