"""Generators of the hand-placed instruction streams (csrc/*_body.inc).  Each is a plain script over the shared `emit`
module -- `python mixgrpo_amd/csrc/gen/<name>.py` -- and is imported by its bare name with this directory on the path, by
the tests and by `generators()` alike, so that there is one module object per generator however it was reached."""
import importlib
import os
import sys

GENERATORS = ("attn_fwd64", "attn_bwd_dq64", "attn_bwd_dkv64")
# (each generator's write() keeps all of its bodies current; the backward's two masked-tail bodies, *kv_body.inc, are build
# products that only build._generate() writes -- .gitignore --, the others are committed)


def generators():
    """The generator modules; each has write() (rewrite its files if their text changed), render() and generate()."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    try:
        return [importlib.import_module(name) for name in GENERATORS]
    finally:
        sys.path.pop(0)
