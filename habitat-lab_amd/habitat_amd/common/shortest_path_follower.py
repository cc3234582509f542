"""habitat's ShortestPathFollower for the Nav2D tasks that have a geodesic field: the oracle agent.  `get_next_actions()` is the
env's `follower_actions()`, one action per env, computed on the device (csrc/nav2d.hip: nav2d_follow_kernel; the rule is stated in
tests/nav2d_follow_reference.py).  `evaluate(num_episodes)` runs that agent on the env's device path and reports what a perfect
agent scores: the oracle row of a results table, a check of the SPL measure, a teacher."""
from typing import Dict

import torch

from habitat_amd import _lib

GO, ARRIVED, UNREACHABLE, STUCK = 0, 1, 2, 3   # include/habitat_amd.h: HAB_NAV2D_FOLLOW_*


class ShortestPathFollower:
    """`envs` is a Nav2DVectorEnv or Nav2DVelVectorEnv in the geodesic distance mode; any other env is refused by name."""

    def __init__(self, envs):
        if not hasattr(envs, "follower_actions"):
            raise _lib.HabError(f"ShortestPathFollower: {type(envs).__name__} has no shortest-path follower")
        if envs._follow_entry is None or envs.distance != "geodesic":
            envs.follower_actions()          # raises, naming the task and the reason
        self.envs = envs
        N, dev = envs.num_envs, envs._state.device
        self._actions = torch.zeros((N, *envs._follow_shape), dtype=envs._action_dtype, device=dev)
        self._next_d = torch.zeros(N, device=dev)
        self._status = torch.zeros(N, dtype=torch.int32, device=dev)
        self._reward, self._not_done = torch.zeros(N, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev)

    def get_next_actions(self, mask=None):
        """The follower's action for every env (for those `mask` selects): the env's tensor, valid until the next call."""
        return self.envs.follower_actions(out=self._actions, mask=mask, next_d=self._next_d, status=self._status)

    @property
    def status(self):
        """int32 (N,): 0 GO, 1 ARRIVED, 2 UNREACHABLE, 3 STUCK of the last `get_next_actions`."""
        return self._status

    @property
    def next_distance(self):
        """float32 (N,): the distance the env reports after the step of a GO; D_PREV where ARRIVED; +inf otherwise."""
        return self._next_d

    def evaluate(self, num_episodes: int) -> Dict[str, float]:
        """Resets the env and steps every env with the follower's actions, without images, until at least `num_episodes` episodes
        have ended.  Returns the means of the env's measures over ALL episodes that ended by then, and the counts: `episodes`,
        `unreachable` and `stuck` (episodes the follower gave up at once / on the way; each ends by the stop it emits), `steps` (env
        steps in all)."""
        if int(num_episodes) <= 0:
            raise _lib.HabError(f"ShortestPathFollower: num_episodes {num_episodes!r} must be positive")
        envs = self.envs
        dev = envs._state.device
        before = envs.measure_sums.double().clone()
        counts = torch.zeros(3, dtype=torch.int64, device=dev)      # episodes, unreachable, stuck
        envs.reset_into_obs({})
        steps = 0
        while True:
            actions = self.get_next_actions()
            counts[1] += (self._status == UNREACHABLE).sum()
            counts[2] += (self._status == STUCK).sum()
            envs.step_into_obs({}, self._reward, self._not_done, actions=actions)
            counts[0] += (self._not_done == 0).sum()
            steps += envs.num_envs
            if int(counts[0]) >= int(num_episodes):    # one read a step: an evaluation, not a rollout
                break
        episodes, unreachable, stuck = (int(v) for v in counts.cpu())
        sums = (envs.measure_sums.double() - before).sum(1).cpu()
        out = {k: float(sums[i]) / episodes for i, k in enumerate(envs.measure_names)}
        out.update(episodes=episodes, unreachable=unreachable, stuck=stuck, steps=steps)
        return out
