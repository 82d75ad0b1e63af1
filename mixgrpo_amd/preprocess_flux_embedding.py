"""Prompt file -> the cached text-embedding dataset of the GRPO trainer, the job of the reference's
fastvideo/data_preprocess/preprocess_flux_embedding.py:83-115 (`FluxPipeline.encode_prompt` per prompt, three .pt files and an
entry of prompt.json), on this package's text encoders (text_encoders.FluxPromptEncoder):

    python -m mixgrpo_amd.preprocess_flux_embedding --model_path <flux dir> --prompt_path <file> --output_dir <dir>
                                                    [--train_batch_size N]

The prompt file is a .txt with one prompt per line (empty lines skipped) or a .json list of strings or of objects with a
`caption`.  (The reference reads its --prompt_path through `get_all_data`, which calls json.loads on the path itself and
cannot run as shipped.)  The output is exactly the layout in the docstring of latent_flux_rl_datasets.py: one file per prompt,
named by the prompt's index in the file, each with the leading dimension of 1 that `encode_prompt` returns, and prompt.json in
file order.  With WORLD_SIZE > 1 (torchrun) rank r takes the prompts r, r + WORLD_SIZE, ...; rank 0 writes prompt.json after
a barrier.  A single process creates no process group.  The reference script's other flags are accepted and ignored."""
import argparse
import json
import os

import torch


def read_prompts(path):
    """-> list of prompts, in file order"""
    with open(path) as f:
        if str(path).endswith(".json"):
            data = json.load(f)
            if not isinstance(data, list):
                raise ValueError(f"{path}: expected a JSON list of strings or of objects with a caption")
            out = []
            for i, e in enumerate(data):
                if isinstance(e, dict) and "caption" in e:
                    e = e["caption"]
                if not isinstance(e, str):
                    raise ValueError(f"{path}: entry {i} is neither a string nor an object with a caption")
                out.append(e)
            return out
        return [line.strip() for line in f if line.strip()]


def write_cache(encoder, prompts, output_dir, batch_size=1, rank=0, world_size=1, barrier=None):
    """Encode this rank's share of `prompts` (indices rank, rank + world_size, ...) in batches and write their files; rank 0
    then writes prompt.json for ALL prompts (after `barrier()`, if given).  `encoder.encode_prompt(list) -> (prompt_embeds
    [B, S, D], pooled [B, W], text_ids [S, 3])`.  Returns the path of prompt.json."""
    subs = ("prompt_embed", "pooled_prompt_embeds", "text_ids")
    for s in subs:
        os.makedirs(os.path.join(output_dir, s), exist_ok=True)
    mine = list(range(rank, len(prompts), world_size))
    for b0 in range(0, len(mine), max(1, batch_size)):
        idx = mine[b0:b0 + max(1, batch_size)]
        embeds, pooled, text_ids = encoder.encode_prompt([prompts[i] for i in idx])
        if embeds.shape[0] != len(idx) or pooled.shape[0] != len(idx):
            raise ValueError(f"encode_prompt returned {tuple(embeds.shape)} / {tuple(pooled.shape)} for {len(idx)} prompts")
        for j, i in enumerate(idx):
            for s, t in zip(subs, (embeds[j:j + 1], pooled[j:j + 1], text_ids)):
                torch.save(t.detach().cpu().clone(), os.path.join(output_dir, s, f"{i}.pt"))
    if barrier is not None:
        barrier()
    path = os.path.join(output_dir, "prompt.json")
    if rank == 0:
        entries = [{"prompt_embed_path": f"{i}.pt", "pooled_prompt_embeds_path": f"{i}.pt", "text_ids": f"{i}.pt", "caption": p}
                   for i, p in enumerate(prompts)]
        with open(path, "w") as f:
            json.dump(entries, f, indent=4)
    return path


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--model_path", type=str, required=True, help="FLUX checkpoint directory (text_encoder/, text_encoder_2/, tokenizer/, tokenizer_2/)")
    p.add_argument("--prompt_path", type=str, required=True)
    p.add_argument("--output_dir", type=str, required=True)
    p.add_argument("--train_batch_size", type=int, default=1)
    # the reference script's other flags: accepted, ignored
    p.add_argument("--model_type", type=str, default=None)
    p.add_argument("--dataloader_num_workers", type=int, default=1)
    p.add_argument("--text_encoder_name", type=str, default=None)
    p.add_argument("--cache_dir", type=str, default=None)
    p.add_argument("--vae_debug", action="store_true")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", rank))
    barrier = None
    if world > 1:
        import torch.distributed as dist
        if not dist.is_initialized():
            dist.init_process_group(backend="gloo", init_method="env://", world_size=world, rank=rank)   # a barrier is all it does
        barrier = dist.barrier
    from .text_encoders import FluxPromptEncoder
    torch.cuda.set_device(local)
    encoder = FluxPromptEncoder.from_pretrained(args.model_path, device=f"cuda:{local}")
    prompts = read_prompts(args.prompt_path)
    path = write_cache(encoder, prompts, args.output_dir, args.train_batch_size, rank, world, barrier)
    if rank == 0:
        print(f"wrote {len(prompts)} prompts to {path}")


if __name__ == "__main__":
    main()
