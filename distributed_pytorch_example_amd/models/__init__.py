"""Model zoo: the reference's SimpleNet plus the BASELINE-scope ResNet-50 and GPT-2-small, and ViT (vit.py)."""
from .simplenet import SimpleNet
from .resnet import ResNet, resnet50, resnet18_like


# ViT-B/16 (86,567,656 parameters), ViT-S/16 (22,050,664); vit-tiny: 2 layers, 17 tokens of a 32 x 32 image
VIT_MODELS = {"vit-b16": dict(n_layer=12, n_head=12, n_embd=768), "vit-s16": dict(n_layer=12, n_head=6, n_embd=384),
              "vit-tiny": {}}


def get_model(name: str, **kw):
    name = name.lower()
    if name == "simplenet":
        return SimpleNet(**kw)
    if name == "resnet50":
        return resnet50(**kw)
    if name in ("resnet_tiny", "resnet18_like"):
        return resnet18_like(**kw)
    if name in ("gpt2", "gpt2-small", "gpt2_small"):
        from .gpt2 import GPT2, GPT2Config

        return GPT2(GPT2Config(**kw))
    if name in ("gpt2-tiny", "gpt2_tiny"):
        from .gpt2 import GPT2, GPT2Config

        return GPT2(GPT2Config.tiny(**kw))
    if name in VIT_MODELS:
        from .vit import ViT, ViTConfig

        if name == "vit-tiny":
            return ViT(ViTConfig.tiny(**kw))
        return ViT(ViTConfig(**{**VIT_MODELS[name], **kw}))
    raise ValueError(f"unknown model {name!r}")


__all__ = ["SimpleNet", "ResNet", "resnet50", "resnet18_like", "get_model"]
