"""``Agent`` / ``MovingAgent`` with the interface of ``sorrel/agents/agent.py:14-225``.

One ``Agent`` object stands for one agent *slot* in every env of the batch: its
``pov`` returns ``[E, ...]`` observations, ``get_action`` returns ``[E]`` actions and
``act`` returns ``[E]`` rewards.  ``transition`` keeps the reference's order
(pov -> get_action -> act -> is_done -> memory), which is what makes
"agent i+1 observes agent i's move" hold for policy-driven agents."""
from __future__ import annotations

from abc import abstractmethod

import torch

from sorrel_amd.entities.entity import Entity


class Agent(Entity):
    """Abstract agent.  ``has_transitions`` defaults to True as in the reference; the
    entity sweep skips agents (``sorrel/environment.py:90``)."""

    def __init__(self, observation_spec, action_spec, model, location=None):
        self.observation_spec = observation_spec
        self.action_spec = action_spec
        self.model = model
        self._location = location
        super().__init__()            # (the reference also resets _location to None here)
        self.has_transitions = True
        self.slot = None              # index in Environment.agents, set by the Environment
        self._world = None

    # -- abstract hooks (sorrel/agents/agent.py:57-111)
    @abstractmethod
    def reset(self) -> None: ...

    @abstractmethod
    def pov(self, world): ...

    @abstractmethod
    def get_action(self, state): ...

    @abstractmethod
    def act(self, world, action): ...

    @abstractmethod
    def is_done(self, world) -> bool: ...

    def type_key(self):
        # an agent's transition is its own step, never a sweep rule
        return (type(self).__module__, type(self).__qualname__, self.kind, float(self.value), bool(self.passable),
                False, None)

    @property
    def locations(self) -> torch.Tensor:
        """``[E, 3]`` (y, x, z) of this agent in every env."""
        w = self._world
        yx = w.agent_pos[:, self.slot].long()
        z = torch.full((yx.shape[0], 1), w.agent_layer, dtype=torch.long, device=yx.device)
        return torch.cat([yx, z], dim=1)

    @property
    def location(self) -> tuple:
        """Location in env 0 (the reference's single world); see ``locations`` for the batch."""
        if self._world is not None and self._world.agent_pos is not None and self.slot is not None \
                and self._world.agent_layer is not None:
            y, x = (int(v) for v in self._world.agent_pos[0, self.slot])
            return (y, x, self._world.agent_layer)
        if self._location is None:
            raise AttributeError(f"{self.kind} location is None.")
        return self._location

    @location.setter
    def location(self, value):
        self._location = value

    #: ``pov`` is the flattened window of the agent's observation spec and ``get_action`` is ``model.take_action`` of it (plus nothing
    #: the host computes per agent): the Environment may then evaluate the policies of many agents in one batch per model and let the
    #: engine sort out whose window an earlier agent's move changed (``Environment.speculate_turns``).  Off unless a class says so.
    speculative_ok = False

    #: action indices after which the agent shows ``sprite_directions[action]`` (the reference sets ``agent.sprite`` inside
    #: ``movement(action)``): None = every action, () = never.  Read by ``sorrel_amd.utils.visualization``; the step kernels do not know it.
    sprite_switch_actions = ()

    def sprite_table(self) -> dict:
        """kind -> list of sprites indexed by action, for every kind (state) this agent can have; one kind unless the sprite list
        depends on the agent's state (Tag).  An entry is a sprite file path, a uint8 ``(th, tw, 4)`` array, or None (the flat tile of
        the kind)."""
        return {self.kind: list(getattr(self, "sprite_directions", ()))}

    def row_tail(self, world):
        """What ``pov`` appends behind the flattened window, as the engine can write it itself (``sgw_bind_row_tail``):
        ``(N.TAIL_AGENT_IS_IT, None)``, ``(N.TAIL_POSITION_TABLE, float32 table [H, W, n])``, or None (``pov`` appends nothing, or
        something only the host can compute)."""
        return None

    def add_memory(self, state, action, reward, done) -> None:
        mem = getattr(self.model, "memory", None)
        if mem is not None:
            mem.add(state, action, reward, done)

    def model_take_action(self, state):
        return self.model.take_action(state)

    def transition(self, world) -> None:
        """pov -> get_action -> act -> is_done -> memory (``agent.py:155-173``).
        ``world.total_reward += reward`` happens inside the step kernel, in agent order."""
        state = self.pov(world)
        action = self.get_action(state)
        reward = self.act(world, action)
        if not torch.is_tensor(action) or action.dim() == 2:
            # get_action returned action VALUES ([E, n_actions]): the act chose -- argmax, or the engine's uniform draw with
            # probability ``epsilon`` (iqn.py:294-309, in-kernel) -- and what it took is on record; or a distribution (ActionProbs /
            # ActionLogits): the engine sampled it (ppo.py:121-137), and a RolloutBuffer receives (action, log_prob)
            action = world._environment._memory_action(self, action)
        done = self.is_done(world)
        self.add_memory(state, action, reward, done)

    @property
    def epsilon(self) -> float:
        """Exploration rate of an agent whose ``get_action`` returns action values: the model's (``iqn.py:305-309``), 0 without one;
        assigning to it overrides the model's."""
        own = self.__dict__.get("_epsilon")
        return float(own) if own is not None else float(getattr(self.model, "epsilon", 0.0) or 0.0)

    @epsilon.setter
    def epsilon(self, value) -> None:
        self.__dict__["_epsilon"] = value


class MovingAgent(Agent):
    """Agent that moves up / down / left / right (``agent.py:176-225``)."""

    direction = 2
    #: what the agent shows after ``movement(action)``, indexed by the ACTION number as in the reference (``agent.py:179-198``: up, down,
    #: left, right).  An entry is a sprite file path, a uint8 ``(th, tw, 4)`` array, or None = the flat tile of the agent's kind (this
    #: package ships no image files).  An action index beyond the list keeps the current sprite (the reference raises IndexError).
    sprite_directions = [None, None, None, None]
    #: ``MovingAgent.act`` calls ``movement`` for every action; a subclass whose ``act`` does not says which actions do
    sprite_switch_actions = None

    def movement(self, action):
        """New location for an action: an int gives the env-0 tuple (reference call shape),
        a tensor ``[E]`` gives ``[E, 3]``.  Any other action name stays in place."""
        names = self.action_spec.actions
        delta = {"up": (-1, 0), "down": (1, 0), "left": (0, -1), "right": (0, 1)}
        if isinstance(action, int):
            dy, dx = delta.get(names[action], (0, 0))
            y, x, z = self.location
            return (y + dy, x + dx, z)
        table = torch.tensor([delta.get(names[i], (0, 0)) + (0,) for i in range(self.action_spec.n_actions)],
                             device=action.device)
        return self.locations + table[action.long()]

    def act(self, world, action):
        """reward = value of the target BEFORE the move, then ``world.move`` -- one
        ``sgw_step`` phase for this agent slot; returns rewards ``[E]``."""
        return world._environment._act(self, action)
