"""Stand-ins for the refiner tests: a deterministic text encoder with the call surface encode_prompt uses
(`enc(ids, output_hidden_states=True)` -> [0] = pooled / projected, `.hidden_states`), a tokenizer without a vocabulary,
and a UNet that records what it was called with.  Test infrastructure only."""
from types import SimpleNamespace

import torch


class StubTokenizer:
    model_max_length = 77

    def __call__(self, texts, padding=None, max_length=77, truncation=True, return_tensors="pt"):
        texts = [texts] if isinstance(texts, str) else texts
        ids = torch.zeros(len(texts), max_length, dtype=torch.long)
        for i, t in enumerate(texts):
            codes = [1] + [3 + (ord(c) % 90) for c in t][: max_length - 2] + [99]
            ids[i, : len(codes)] = torch.tensor(codes)
        return SimpleNamespace(input_ids=ids)


class _Out(tuple):
    hidden_states = None


class StubTextEncoder:
    """Three tanh layers over an embedding table; [0] is the last layer at the end token times a projection."""

    def __init__(self, hidden, proj, seed):
        g = torch.Generator().manual_seed(seed)
        self.emb = torch.randn(100, hidden, generator=g)
        self.mix = [torch.randn(hidden, hidden, generator=g) / hidden ** 0.5 for _ in range(3)]
        self.proj = torch.randn(hidden, proj, generator=g) / hidden ** 0.5
        self.calls = 0
        self.final_layer_norm = lambda x: x          # (read by encode_prompt's clip_skip branch; unused for SDXL)

    def to(self, device):
        self.emb, self.proj = self.emb.to(device), self.proj.to(device)
        self.mix = [m.to(device) for m in self.mix]
        return self

    def __call__(self, ids, output_hidden_states=False):
        self.calls += 1
        h = self.emb[ids]
        hs = [h]
        for m in self.mix:
            h = torch.tanh(h @ m)
            hs.append(h)
        pooled = h[torch.arange(ids.shape[0], device=ids.device), ids.argmax(dim=-1)] @ self.proj
        out = _Out((pooled, h))
        out.hidden_states = tuple(hs)
        return out


class RecordingUNet:
    """The `.base` / `.refiner` call surface without a network: returns 0.1 * sample, records (t, added conditions)."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.config = SimpleNamespace(**cfg.to_dict())
        self.dtype = torch.float32
        self.add_embedding = SimpleNamespace(linear_1=SimpleNamespace(in_features=cfg.projection_class_embeddings_input_dim))
        self.calls = []
        self.device = "cpu"

    def to(self, device):
        self.device = str(device)
        return self

    def __call__(self, sample, t, ehs, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False):
        self.calls.append(SimpleNamespace(t=float(t), sample=tuple(sample.shape), ehs=tuple(ehs.shape),
                                          text_embeds=added_cond_kwargs["text_embeds"].clone(),
                                          time_ids=added_cond_kwargs["time_ids"].clone()))
        return (0.1 * sample[:, :4],)
