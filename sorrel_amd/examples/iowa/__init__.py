"""Iowa Gambling Task (``sorrel/examples/iowa``) on the batched engine: four decks whose payoff is redrawn every turn."""
