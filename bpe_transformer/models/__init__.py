"""Model zoo: decoder-only Transformer LM and its building blocks."""

from . import functional
from .config import PRESETS, ModelConfig, get_preset
from .layers import (
    ActFFN,
    Embedding,
    Linear,
    MultiHeadSelfAttention,
    RMSNorm,
    RotaryPositionalEmbedding,
    SwiGLU,
    TransformerBlock,
)
from .generation import DecodeSession, KVCache, PromptLookupSession, SpeculativeSession
from .serving import RequestOutput, SamplingParams, ServingEngine
from .transformer import TransformerLM

__all__ = [
    "PRESETS",
    "ActFFN",
    "DecodeSession",
    "Embedding",
    "KVCache",
    "Linear",
    "ModelConfig",
    "MultiHeadSelfAttention",
    "PromptLookupSession",
    "RMSNorm",
    "RequestOutput",
    "RotaryPositionalEmbedding",
    "SamplingParams",
    "ServingEngine",
    "SpeculativeSession",
    "SwiGLU",
    "TransformerBlock",
    "TransformerLM",
    "functional",
    "get_preset",
]
