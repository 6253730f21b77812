from sorrel_amd.models.base_model import ActionLogits, ActionProbs, BaseModel, RandomModel
from sorrel_amd.models.iqn import IQN, IQNActor, IQNOutput, NoisyLinear
from sorrel_amd.models.iqn_learner import iRainbowModel

PyTorchIQN = iRainbowModel                    # (the name the reference's examples import: sorrel.models.pytorch.PyTorchIQN)

__all__ = ["ActionLogits", "ActionProbs", "BaseModel", "RandomModel", "IQN", "IQNActor", "IQNOutput", "NoisyLinear", "iRainbowModel", "PyTorchIQN"]
