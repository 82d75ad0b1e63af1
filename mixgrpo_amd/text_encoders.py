"""Prompts -> what the FLUX transformer and the cached dataset take: diffusers' `FluxPipeline.encode_prompt`, which the
reference's fastvideo/data_preprocess/preprocess_flux_embedding.py:89 calls, on this package's text encoders (t5.py,
clip_text.py).

Tokenising stays on the host and is delegated: `load_tokenizer(dir, max_length)` lazily imports transformers' AutoTokenizer
(never at package import) and returns a callable `prompts -> int tensor [B, max_length]`; any callable of that shape is accepted
in its place everywhere a tokenizer is asked for (tests use stubs: no vocabulary file exists offline)."""
import os

import torch


def load_tokenizer(path, max_length):
    """A tokenizer directory -> `prompts -> input_ids [B, max_length]` (int64, host), padded to `max_length` and truncated to
    it: CLIP's convention at 77, T5's at 512, as `encode_prompt` tokenises for both."""
    from transformers import AutoTokenizer
    tok = AutoTokenizer.from_pretrained(path)

    def tokenize(prompts):
        return tok(list(prompts), padding="max_length", max_length=max_length, truncation=True, return_tensors="pt").input_ids
    return tokenize


def as_tokenizer(tokenizer, max_length):
    """A directory name -> `load_tokenizer`; a callable as it is."""
    if callable(tokenizer):
        return tokenizer
    return load_tokenizer(tokenizer, max_length)


class FluxPromptEncoder:
    """`encode_prompt(prompts)` as FluxPipeline's: T5 `last_hidden_state` of `tokenizer_2`'s ids, the CLIP text model's
    `pooler_output` of `tokenizer`'s ids, and zero text ids."""

    def __init__(self, clip_tower, t5_encoder, clip_tokenizer, t5_tokenizer, t5_max_length=512):
        self.clip, self.t5 = clip_tower, t5_encoder
        self.clip_tokenizer = as_tokenizer(clip_tokenizer, clip_tower.config.context)
        self._t5_tokenizer, self._t5_tok = t5_tokenizer, {}
        self.t5_max_length = t5_max_length
        self.device = t5_encoder.device

    @classmethod
    def from_pretrained(cls, flux_dir, device="cuda"):
        """A FLUX checkpoint directory: `text_encoder/` (CLIP-L text model), `text_encoder_2/` (T5-XXL), `tokenizer/`,
        `tokenizer_2/`."""
        from .clip_text import ClipTextTower
        from .t5 import T5Encoder
        d = lambda n: os.path.join(flux_dir, n)
        return cls(ClipTextTower.from_pretrained(d("text_encoder"), device), T5Encoder.from_pretrained(d("text_encoder_2"), device),
                   d("tokenizer"), d("tokenizer_2"))

    def _t5_tokenize(self, prompts, max_length):
        if callable(self._t5_tokenizer):
            return self._t5_tokenizer(prompts)
        if max_length not in self._t5_tok:
            self._t5_tok[max_length] = load_tokenizer(self._t5_tokenizer, max_length)
        return self._t5_tok[max_length](prompts)

    @torch.no_grad()
    def encode_prompt(self, prompts, max_sequence_length=None):
        """-> (prompt_embeds [B, S, d_model] bf16, pooled_prompt_embeds [B, width] bf16, text_ids zeros [S, 3] bf16), S =
        max_sequence_length (512): [B, 512, 4096] / [B, 768] / [512, 3] for FLUX."""
        if isinstance(prompts, str):
            prompts = [prompts]
        prompts = list(prompts)
        S = max_sequence_length or self.t5_max_length
        ids2 = self._t5_tokenize(prompts, S)
        if tuple(ids2.shape) != (len(prompts), S):
            raise ValueError(f"the T5 tokenizer returned {tuple(ids2.shape)} for {len(prompts)} prompts at max_length {S}")
        pooled = self.clip.pooled_output(self.clip_tokenizer(prompts))
        embeds = self.t5.encode(ids2)
        return embeds, pooled, torch.zeros(S, 3, dtype=embeds.dtype, device=embeds.device)
