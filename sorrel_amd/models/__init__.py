from sorrel_amd.models.base_model import ActionLogits, ActionProbs, BaseModel, RandomModel

__all__ = ["ActionLogits", "ActionProbs", "BaseModel", "RandomModel"]
