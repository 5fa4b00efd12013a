"""Operation mixin for the door task (envs/operation/OperationMujocoUR5eDoor.py:1-22): env
construction and the scripted pre-rollout phase Grasp with the gripper opened
(GraspPhaseBase.set_target_open = action_space.low, PhaseBase.py:81-82), 0.5 s."""

from ...common.rollout_base import PhaseSpec
from ..ur5e_door import BatchedMujocoUR5eDoorEnv


class OperationMujocoUR5eDoor:
    def setup_env(self, render_mode=None):
        self.env = BatchedMujocoUR5eDoorEnv(
            self.args.num_envs, self.args.device, world_random_scale=self.args.world_random_scale, seed=self.args.seed,
            env_offset=self.args.env_offset, shadows=getattr(self.args, "shadows", "off"),
            offsamples=getattr(self.args, "offsamples", 1),
        )

    def get_pre_motion_phases(self):
        return [PhaseSpec("GraspPhase", 0.5, "grasp", grip="low")]
