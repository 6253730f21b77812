"""``GamblingEnv`` (``sorrel/examples/iowa/env.py:28-224``) on the batched engine."""
from sorrel_amd.action.action_spec import ActionSpec
from sorrel_amd.environment import Environment
from sorrel_amd.examples.iowa.agents import GamblingAgent
from sorrel_amd.examples.iowa.entities import DECK_KINDS, EmptyEntity, Sand, Wall
from sorrel_amd.models import RandomModel
from sorrel_amd.observation.observation_spec import OneHotObservationSpec

ENTITY_LIST = ["EmptyEntity", "Wall", "Sand", "DeckA", "DeckB", "DeckC", "DeckD", "GamblingAgent"]


class GamblingEnv(Environment):
    """config keys: ``world.{height,width,spawn_prob}``, ``model.agent_vision_radius``, optional ``model.num_agents`` (default 2)."""

    record_targets = True        # the engine records what every agent stepped on in the last turn (``env.target_types``)
    record_encounters = tuple(DECK_KINDS)    # ... and counts the decks among it: ``env.encounters``, int64 [E, A, 4], added to by the acts themselves

    def __init__(self, world, config, model_factory=None):
        self._model_factory = model_factory
        super().__init__(world, config)

    def setup_agents(self):
        n = int(self.config.model.get("num_agents", 2))
        agents = []
        for _ in range(n):
            ospec = OneHotObservationSpec(ENTITY_LIST, full_view=False, vision_radius=int(self.config.model.agent_vision_radius))
            size = 1
            for d in ospec.input_size:
                size *= d
            ospec.override_input_size((size,))
            aspec = ActionSpec(["up", "down", "left", "right"])
            if self._model_factory is not None:
                model = self._model_factory(ospec.input_size, aspec.n_actions)
            else:
                model = RandomModel(ospec.input_size, aspec.n_actions)
            agents.append(GamblingAgent(ospec, aspec, model))
        self.agents = agents

    def populate_environment(self):
        """Walls around BOTH layers, sand below, spawning EmptyEntity on the top layer, agents on distinct random interior
        cells of it (``env.py:93-124``) -- declared once, executed by the reset kernel for every env."""
        self.world.set_layout(layer_fill=[Sand(), EmptyEntity()], layer_border=[Wall(), Wall()])
        self.spawn_agents()

    # ------------------------------------------------------------------ encounters
    # GamblingAgent.act's bookkeeping (agents.py:54-56) is done by the engine's acts (sgw_bind_encounters): fresh and drawn deck twins share
    # their kind's slot, everything else is uncounted.  Nothing is folded on the host, so rollout() is Environment.rollout: one launch.

    def run_experiment(self, animate: bool = False, logging: bool = True, logger=None, output_dir=None, epochs=None, max_turns=None,
                       all_reduce: bool = True):
        """The reference's epoch loop (``env.py:126-224``): ``Environment.run_experiment``, plus the encounters of all agents and envs
        per deck in every epoch's record -- ``history[epoch]["encounters"]`` and ``logger.record_turn(..., encounters=...)``."""
        outer = self

        class _WithEncounters:
            def record_turn(self, epoch, loss, reward, epsilon):
                logger.record_turn(epoch, loss, reward, epsilon, encounters=outer.encounter_counts())

        self._epoch_encounters = []
        history = super().run_experiment(animate=animate, logging=logging, logger=_WithEncounters() if logger is not None else None,
                                         output_dir=output_dir, epochs=epochs, max_turns=max_turns, all_reduce=all_reduce)
        for m, enc in zip(history, self._epoch_encounters[1:] + [self.encounter_counts()]):
            m["encounters"] = enc
        self._epoch_encounters = None
        return history

    def encounter_counts(self) -> dict:
        """``{"DeckA": n, ...}`` over all agents and envs of the epoch so far (synchronising)."""
        return {k: int(v) for k, v in zip(DECK_KINDS, self.encounters.sum(dim=(0, 1)).tolist())}

    def reset(self) -> None:
        if getattr(self, "_epoch_encounters", None) is not None:
            self._epoch_encounters.append(self.encounter_counts())     # (what the epoch that ends here counted)
        super().reset()
