"""``GamblingAgent`` (``sorrel/examples/iowa/agents.py:15-65``), batched."""
import torch

from sorrel_amd.agents import MovingAgent
from sorrel_amd.examples.iowa.entities import DECK_KINDS


class GamblingAgent(MovingAgent):
    speculative_ok = True        # pov = the flattened window, get_action = model.take_action

    def __init__(self, observation_spec, action_spec, model):
        super().__init__(observation_spec, action_spec, model)

    @property
    def encounters(self) -> torch.Tensor:
        """How often this agent stepped on each deck this epoch, per env: int64 ``[E, 4]`` in ``DECK_KINDS`` order (the
        reference's dict, ``agents.py:22``, for every env of the batch).  Counted by the engine's acts into the environment's tensor
        (``Environment.record_encounters``); ``reset()`` clears it, as the reference's does."""
        return self._world._environment.encounters[:, self.slot]

    def encounter_counts(self) -> dict:
        """The reference's ``{"DeckA": n, ...}``, summed over the batch (synchronising)."""
        total = self.encounters.sum(dim=0).tolist()
        return {k: int(v) for k, v in zip(DECK_KINDS, total)}

    def reset(self) -> None:
        self.model.reset()
        if self._world is not None and self.slot is not None:
            self.encounters.zero_()

    def pov(self, world) -> torch.Tensor:
        image = self.observation_spec.observe(world, self)
        return image.reshape(image.shape[0], -1)

    def get_action(self, state: torch.Tensor) -> torch.Tensor:
        mem = getattr(self.model, "memory", None)
        if mem is not None and mem.n_frames > 1:
            prev = mem.current_state()                                   # [n_frames-1, E, obs]
            state = torch.cat([prev.permute(1, 0, 2).reshape(state.shape[0], -1), state], dim=1)
        return self.model.take_action(state)

    # act() is MovingAgent.act: reward = the value the target has THIS turn, read before the move

    def is_done(self, world) -> bool:
        return world.is_done
