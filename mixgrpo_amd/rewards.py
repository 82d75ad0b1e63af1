"""The reference's three CLIP rewards on the HIP image tower (mixgrpo_amd/clip_vision.py):

    kind                    score                                       reference
    HPSClipRewardModel      cosine(image, text)                         hps_score.py:70-77 (normalised features, no logit scale)
    CLIPScoreRewardModel    cosine(image, text)                         clip_score.py:63-70
    PickScoreRewardModel    (exp(logit_scale) * cosine - mean) / std    pick_score.py:73-82

(files under fastvideo/models/reward_model/).  A prompt's text feature is constant.  It comes from one of two objects with the
same `lookup(prompts, device)`:
    TextTowerFeatures   encodes a prompt the first time it is seen, on the HIP text tower (mixgrpo_amd/clip_text.py) with a
                        delegated tokenizer, and memoises it: no offline step, as the reference's models, which take
                        `(images, prompts)` and encode the prompt themselves (hps_score.py:69-72, pick_score.py:64-77);
    TextFeatureCache    looks it up in a file computed once, offline, with whatever text tower the user owns
                        (`build_text_feature_cache`); an unknown prompt is a KeyError.
Only the image tower runs on every step of the training loop: `decode -> ClipReward` stays on the device, with no PIL image and
no host copy of one.

The reference's fourth local reward, ImageRewardModel (image_reward.py:24-40), is not a CLIP: mixgrpo_amd/image_reward.py holds
it, and `builtin_rewards` builds it from an entry of its own (IMAGE_REWARD).

`builtin_rewards` is a factory for `--mgx_reward_plugin mixgrpo_amd.rewards:builtin_rewards`."""
import json
import os

import torch

from . import ops

KINDS = ("HPSClipRewardModel", "CLIPScoreRewardModel", "PickScoreRewardModel")
IMAGE_REWARD = "ImageRewardModel"            # not one of KINDS: no ClipReward, an image_reward.ImageRewardModel
CONFIG_ENV = "MGX_REWARD_CONFIG"


def build_text_feature_cache(prompts, encode_text, path, batch_size=64):
    """Write the cache `TextFeatureCache` reads: `encode_text(list of prompts) -> [n, embed]` tensor (any text tower), one row
    per distinct prompt.  `path` ends in .safetensors (the prompts go into the file's metadata as a JSON list) or .pt (a dict
    with `features` and `prompts`)."""
    prompts = list(dict.fromkeys(prompts))
    rows = [torch.as_tensor(encode_text(prompts[i:i + batch_size])).detach().float().cpu() for i in range(0, len(prompts), batch_size)]
    feats = torch.cat(rows).contiguous()
    if feats.dim() != 2 or feats.shape[0] != len(prompts):
        raise ValueError(f"encode_text returned {tuple(feats.shape)} for {len(prompts)} prompts")
    if str(path).endswith(".safetensors"):
        from safetensors.torch import save_file
        save_file({"features": feats}, str(path), metadata={"prompts": json.dumps(prompts)})
    else:
        torch.save({"features": feats, "prompts": prompts}, str(path))
    return path


class TextFeatureCache:
    """features [n, embed] + the JSON list of their n prompts, from a .safetensors file (prompts in its metadata, or in a
    `<path>.json` next to it) or a .pt file (dict with `features` and `prompts`)."""

    def __init__(self, path=None, features=None, prompts=None):
        if path is not None:
            features, prompts = self._read(str(path))
        self.features = torch.as_tensor(features).float()
        self.prompts = list(prompts)
        if self.features.dim() != 2 or self.features.shape[0] != len(self.prompts):
            raise ValueError(f"{tuple(self.features.shape)} features for {len(self.prompts)} prompts")
        self.index = {p: i for i, p in enumerate(self.prompts)}
        self._on = {}

    @staticmethod
    def _read(path):
        prompts = None
        if path.endswith(".safetensors"):
            from safetensors import safe_open
            with safe_open(path, "pt") as f:
                features = f.get_tensor("features")
                meta = f.metadata() or {}
            if "prompts" in meta:
                prompts = json.loads(meta["prompts"])
        else:
            d = torch.load(path, map_location="cpu")
            features, prompts = d["features"], d.get("prompts")
        if prompts is None:
            with open(path + ".json") as f:
                prompts = json.load(f)
        return features, prompts

    def rows(self, prompts):
        """Indices of the prompts; an unknown one is a KeyError that quotes it."""
        out = []
        for p in prompts:
            if p not in self.index:
                raise KeyError(f"no cached text feature for the prompt {p!r}: add it with build_text_feature_cache")
            out.append(self.index[p])
        return out

    def lookup(self, prompts, device):
        """[len(prompts), embed] fp32 on `device`"""
        idx = self.rows(prompts)
        device = torch.device(device)
        t = self._on.get(device)
        if t is None:
            t = self._on[device] = self.features.to(device)
        return t[torch.tensor(idx, device=device)].contiguous()


class TextTowerFeatures:
    """`TextFeatureCache`'s `lookup` on a text tower: `text_tower.encode_text(input_ids) -> [n, embed]` (a ClipTextTower) and
    `tokenizer`, a callable `prompts -> int tensor [n, S]` or a tokenizer directory (text_encoders.load_tokenizer).  The unseen
    prompts of a lookup are encoded as one batch and memoised by prompt."""

    def __init__(self, text_tower, tokenizer):
        self.text_tower, self.tokenizer = text_tower, tokenizer
        self._rows = {}

    def lookup(self, prompts, device):
        """[len(prompts), embed] fp32 on `device`"""
        new = [p for p in dict.fromkeys(prompts) if p not in self._rows]
        if new:
            if not callable(self.tokenizer):                   # a directory: transformers is imported on first use only
                from .text_encoders import load_tokenizer
                self.tokenizer = load_tokenizer(self.tokenizer, self.text_tower.config.context)
            feats = self.text_tower.encode_text(self.tokenizer(new)).detach().float()
            if feats.dim() != 2 or feats.shape[0] != len(new):
                raise ValueError(f"encode_text returned {tuple(feats.shape)} for {len(new)} prompts")
            for p, row in zip(new, feats):
                self._rows[p] = row.clone()
        return torch.stack([self._rows[p] for p in prompts]).to(torch.device(device)).contiguous()


class ClipReward:
    """`(images, prompts) -> list[float]`, the order reward_adapter.compute_reward uses.  Images are [3, H, W] device tensors as
    AutoencoderKL.decode returns them (PIL images are converted on the host); `text_features` a TextFeatureCache or a
    TextTowerFeatures."""

    def __init__(self, tower, text_features, kind, mean=18.0, std=8.0):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}, not {kind!r}")
        if kind == "PickScoreRewardModel" and tower.logit_scale is None:
            raise ValueError("PickScoreRewardModel needs the checkpoint's logit_scale, which this tower's state dict did not hold")
        self.tower, self.text_features, self.kind = tower, text_features, kind
        self.mean, self.std = float(mean), float(std)

    def score_params(self):
        """(logit scale, mean, std) of `(scale * cosine - mean) / std`"""
        if self.kind == "PickScoreRewardModel":
            return float(torch.tensor(self.tower.logit_scale).exp()), self.mean, self.std
        return 1.0, 0.0, 1.0

    @torch.no_grad()
    def __call__(self, images, prompts):
        if isinstance(prompts, str):
            prompts = [prompts]
        if torch.is_tensor(images):
            images = list(images) if images.dim() == 4 else [images]
        elif not isinstance(images, (list, tuple)):
            images = [images]
        if len(images) != len(prompts):
            raise ValueError(f"{len(images)} images for {len(prompts)} prompts")
        dev = self.tower.device
        text = self.text_features.lookup(prompts, dev)          # before anything is launched: an unknown prompt is a KeyError
        feats = self.tower.encode_image(images, normalize=False)
        out = torch.empty(len(images), dtype=torch.float32, device=dev)
        ops.cosine_score(feats, text, out, *self.score_params())
        return out.tolist()


def _image_reward(path, c, args):
    from . import image_reward
    files = {"checkpoint": "image_reward_path", "med_config": "image_reward_med_config"}
    given = {k: c.get(k) or getattr(args, a, None) for k, a in files.items()}
    missing = [k for k, v in given.items() if not v]
    if missing:
        raise ValueError(f"{path}: {IMAGE_REWARD} lacks {missing}")
    tok = c.get("tokenizer_dir", os.path.dirname(os.path.abspath(given["checkpoint"])))
    return image_reward.ImageRewardModel.from_pretrained(given["checkpoint"], given["med_config"], tokenizer=tok,
                                                         mean=c.get("mean", image_reward.MEAN), std=c.get("std", image_reward.STD),
                                                         device=c.get("device", "cuda"))


def builtin_rewards(args=None):
    """`--mgx_reward_plugin mixgrpo_amd.rewards:builtin_rewards`: reads the JSON file named by the environment variable
    MGX_REWARD_CONFIG, `{RewardClassName: {"tower_dir": ..., "text_features": ..., ["mean": 18.0, "std": 8.0, "device": "cuda"]}}`,
    and returns `{RewardClassName: ClipReward}`.  Instead of `text_features` (a TextFeatureCache file) an entry may give
    `"text_tower_dir"` (config.json + safetensors of the text tower; the image tower's directory if it holds a whole CLIPModel)
    and optionally `"tokenizer_dir"` (default: the text tower's directory): prompts are then encoded as they come
    (TextTowerFeatures).  Rewards that name the same directory share one tower.
    An `"ImageRewardModel"` entry is `{"checkpoint": ..., "med_config": ..., ["tokenizer_dir", "mean", "std", "device"]}` and gives
    an image_reward.ImageRewardModel; `checkpoint` and `med_config` default to `args.image_reward_path` and
    `args.image_reward_med_config` when `args` carries them, `tokenizer_dir` to the checkpoint's directory."""
    from .clip_vision import ClipVisionTower
    path = os.environ.get(CONFIG_ENV)
    if not path:
        raise ValueError(f"builtin_rewards: set {CONFIG_ENV} to a JSON file {{RewardClassName: {{tower_dir, text_features}}}}")
    with open(path) as f:
        cfg = json.load(f)
    if not isinstance(cfg, dict) or not cfg:
        raise ValueError(f"{path}: expected a non-empty JSON object")
    towers, caches, out = {}, {}, {}
    for name, c in cfg.items():
        if name == IMAGE_REWARD:
            out[name] = _image_reward(path, c, args)
            continue
        if name not in KINDS:
            raise ValueError(f"{path}: {name!r} is not one of {KINDS + (IMAGE_REWARD,)}")
        missing = [k for k in ("tower_dir", "text_features") if k not in c and not (k == "text_features" and "text_tower_dir" in c)]
        if missing:
            raise ValueError(f"{path}: {name} lacks {missing}")
        tkey = (c["tower_dir"], c.get("device", "cuda"))
        if tkey not in towers:
            towers[tkey] = ClipVisionTower.from_pretrained(*tkey)
        if "text_features" in c:
            ckey = c["text_features"]
            if ckey not in caches:
                caches[ckey] = TextFeatureCache(ckey)
        else:
            ckey = (c["text_tower_dir"], c.get("tokenizer_dir", c["text_tower_dir"]), tkey[1])
            if ckey not in caches:
                from .clip_text import ClipTextTower
                caches[ckey] = TextTowerFeatures(ClipTextTower.from_pretrained(ckey[0], ckey[2]), ckey[1])
        out[name] = ClipReward(towers[tkey], caches[ckey], name, c.get("mean", 18.0), c.get("std", 8.0))
    return out
