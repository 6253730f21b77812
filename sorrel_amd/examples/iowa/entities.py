"""Iowa Gambling Task entities (``sorrel/examples/iowa/entities.py``).

The reference's ``Deck.transition`` redraws ``value`` every turn.  Here that is a declarative value rule
(``DrawnValue``): a cell stores a type id, and what a drawn deck is worth in a turn is a function of (seed, env, epoch,
turn, cell) that the act evaluates when an agent steps on it.  A deck the sweep has not visited yet -- the one
``EmptyEntity.transition`` spawned this turn -- still has the constructor's value 0; it is a type of its own (``Deck(name)``,
"fresh") that becomes its drawn twin (``Deck(name, drawn=True)``) on the next sweep.  Both look the same (one kind), as the
aged types of ``AgeRule`` do."""
from sorrel_amd.entities import BecomeIfRule, Entity, SpawnRule
from sorrel_amd.entities.rules import DrawnValue

DECKS = ("a", "b", "c", "d")
DECK_KINDS = tuple(f"Deck{n.upper()}" for n in DECKS)
# base payoff, loss, probability of the loss (Deck.draw, entities.py:45-66): a / b are the bad decks, c / d the good ones
PAYOFF = {"a": (1, -2.5, 0.5), "b": (1, -12.5, 0.1), "c": (0.5, -0.5, 0.5), "d": (0.5, -2.5, 0.1)}


def deck_outcomes(name: str):
    """(value without the loss, value with it, probability of the loss), in Python floats and in the reference's order of
    operations: ``value = base``; ``value += loss``; ``return value + 0.1``."""
    base, loss, prob = PAYOFF[name]
    without = base + 0.1
    value = base
    value += loss
    return without, value + 0.1, prob


_VALUE_RULE = {n: DrawnValue(*deck_outcomes(n)) for n in DECKS}


class Wall(Entity):
    def __init__(self):
        super().__init__()
        self.value = -1   # walls penalise contact


class Sand(Entity):
    def __init__(self):
        super().__init__()
        self.passable = True


class Deck(Entity):
    """``Deck(name)``: as the reference constructs it -- value 0 until its first sweep.  ``drawn=True``: the deck every later
    turn sees; its host-side ``value`` is the outcome without the loss, the per-turn draw is visible through the rewards only."""

    def __init__(self, name: str, drawn: bool = False):
        super().__init__()
        self.passable = True
        self.name = name
        self.drawn = bool(drawn)
        self.kind = f"Deck{name.upper()}"     # different decks are different entities to an observer
        if drawn:
            self.value_rule = _VALUE_RULE[name]
            self.value = _VALUE_RULE[name].otherwise
        else:
            self.value = 0
            self.has_transitions = True
            self.transition_rule = _FIRST_SWEEP[name]


# one rule object per deck: a rule is part of an entity's type, so every fresh Deck("a") is the same type
_FIRST_SWEEP = {n: BecomeIfRule(lambda world, n=n: Deck(n, drawn=True)) for n in DECKS}


class EmptyEntity(Entity):
    """Empty space that may turn into one of the four decks each turn (``entities.py:77-91``)."""

    transition_rule = SpawnRule(prob=lambda world: world.spawn_prob, choices=lambda world: [Deck(n) for n in DECKS])

    def __init__(self):
        super().__init__()
        self.passable = True
        self.has_transitions = True
