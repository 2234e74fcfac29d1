"""Text encoders of the diffusion pipelines (reference: src/pygpukit/diffusion/text_encoders): the reference's class names and
constructor arguments; the computation is HuggingFace's T5EncoderModel and CLIPTextModel, on the device (t5.py, clip.py)."""

from pygpukit_amd.diffusion.text_encoders.clip import CLIPTextEncoder, CLIPTextEncoderG, CLIPTextEncoderL
from pygpukit_amd.diffusion.text_encoders.t5 import T5Encoder, T5XXLEncoder, t5_plan

__all__ = ["CLIPTextEncoder", "CLIPTextEncoderL", "CLIPTextEncoderG", "T5Encoder", "T5XXLEncoder", "t5_plan"]
