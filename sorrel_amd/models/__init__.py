from sorrel_amd.models.base_model import ActionLogits, ActionProbs, BaseModel, RandomModel
from sorrel_amd.models.iqn import IQN, IQNActor, IQNOutput, NoisyLinear

__all__ = ["ActionLogits", "ActionProbs", "BaseModel", "RandomModel", "IQN", "IQNActor", "IQNOutput", "NoisyLinear"]
