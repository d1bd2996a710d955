"""Model zoo: the reference's SimpleNet plus the BASELINE-scope ResNet-50 and GPT-2-small, ViT (vit.py), ConvNeXt
(convnext.py) and the Llama-style decoder (llama.py)."""
from .simplenet import SimpleNet
from .resnet import ResNet, resnet50, resnet18_like


# ViT-B/16 (86,567,656 parameters), ViT-S/16 (22,050,664); vit-tiny: 2 layers, 17 tokens of a 32 x 32 image
VIT_MODELS = {"vit-b16": dict(n_layer=12, n_head=12, n_embd=768), "vit-s16": dict(n_layer=12, n_head=6, n_embd=384),
              "vit-tiny": {}}
# name -> the LlamaConfig constructor (llama.py): TinyLlama-1.1B (1,100,048,384 parameters); llama-tiny: 2 layers, 4 / 2 heads
LLAMA_MODELS = {"tinyllama-1.1b": "tinyllama_1_1b", "llama-tiny": "tiny"}


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
    if name in LLAMA_MODELS:
        from .llama import Llama, LlamaConfig

        return Llama(getattr(LlamaConfig, LLAMA_MODELS[name])(**kw))
    if name in ("convnext-tiny", "convnext-test"):
        from .convnext import ConvNeXt, ConvNeXtConfig

        return ConvNeXt(ConvNeXtConfig.tiny_test(**kw) if name == "convnext-test" else ConvNeXtConfig(**kw))
    raise ValueError(f"unknown model {name!r}")


__all__ = ["SimpleNet", "ResNet", "resnet50", "resnet18_like", "get_model"]
