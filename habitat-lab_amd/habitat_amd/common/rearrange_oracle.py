"""The pick-and-place oracle of Nav2DRearr-v0 in the geodesic distance mode: what a competent agent scores under the task's own
rules.  `get_next_actions()` is the env's `oracle_actions()`, one action per env, computed on the device (csrc/nav2d.hip:
nav2d_rearr_oracle_kernel; the rule is stated in tests/nav2d_rearr_oracle_reference.py): go to the object down the field DO, PICK,
carry it down DG, PLACE where it will rest within the success distance, STOP.  `evaluate(num_episodes)` runs that agent on the env's
device path: the oracle row beside a learning run's `success`, `did_pick_object` and `object_to_goal_distance`, and a check that
both geodesic fields are good enough to act on."""
from typing import Dict

import torch

from habitat_amd import _lib

GO, ARRIVED, UNREACHABLE, STUCK, PICK, PLACE = 0, 1, 2, 3, 4, 5   # include/habitat_amd.h: HAB_NAV2D_ORACLE_*


class RearrangeOracle:
    """`envs` is a Nav2DRearrVectorEnv in the geodesic distance mode; any other env is refused by name."""

    def __init__(self, envs):
        if not hasattr(envs, "oracle_actions"):
            raise _lib.HabError(f"RearrangeOracle: {type(envs).__name__} has no pick-and-place oracle")
        if envs._oracle_entry is None or envs.distance != "geodesic":
            envs.oracle_actions()          # raises, naming the task and the reason
        self.envs = envs
        N, dev = envs.num_envs, envs._state.device
        self._actions = torch.zeros(N, dtype=torch.int64, device=dev)
        self._next_d = torch.zeros(N, device=dev)
        self._status = torch.zeros(N, dtype=torch.int32, device=dev)
        self._reward, self._not_done = torch.zeros(N, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev)

    def get_next_actions(self, mask=None):
        """The oracle's action for every env (for those `mask` selects): the oracle's own tensor, valid until the next call."""
        return self.envs.oracle_actions(out=self._actions, mask=mask, next_d=self._next_d, status=self._status)

    @property
    def status(self):
        """int32 (N,): 0 GO, 1 ARRIVED, 2 UNREACHABLE, 3 STUCK, 4 PICK, 5 PLACE of the last `get_next_actions`."""
        return self._status

    @property
    def next_distance(self):
        """float32 (N,): the leg's term (a not holding, b holding) as the env reports it after the step; +inf where the oracle
        gave up."""
        return self._next_d

    def evaluate(self, num_episodes: int) -> Dict[str, float]:
        """Resets the env and steps every env with the oracle's actions, without images, until at least `num_episodes` episodes
        have ended.  Returns the means of the env's four measures over ALL episodes that ended by then, and the counts: `episodes`,
        `unreachable` and `stuck` (episodes the oracle gave up at once / on the way; each ends by the stop it emits), `steps` (env
        steps in all)."""
        if int(num_episodes) <= 0:
            raise _lib.HabError(f"RearrangeOracle: num_episodes {num_episodes!r} must be positive")
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
