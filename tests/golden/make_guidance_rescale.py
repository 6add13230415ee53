#!/usr/bin/env python3
"""Generates tests/golden/guidance_rescale.npz: outputs of the REFERENCE'S OWN `rescale_noise_cfg`
(pipelines/sd_unified_pipeline.py:46-57 -- defined there and never called) on a few small inputs, so that the product's
restatement in stablediffusion_amd/pipeline.py is pinned to the reference's code instead of to a re-typed copy.

Run in the build container only (needs the reference checkout; the GPU box never runs this):
    python tests/golden/make_guidance_rescale.py

How (same as make_hostlogic.py): the module cannot be imported (diffusers is not installed), but this function is pure
torch.  Its definition is taken out of the file with `ast` (nothing else of the module is executed) and called.  What is
committed is DATA: the inputs and the function's outputs.  No reference source text is stored.
tests/test_guidance_rescale.py compares the product against every case.
"""
import ast
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PIPE = "/root/reference/pipelines/sd_unified_pipeline.py"
PHIS = (0.3, 0.7, 1.0)
# (name, shape, dtype, guidance scale used to build noise_cfg, offset of the text prediction's mean)
CASES = (("a", (2, 4, 8, 8), torch.float32, 7.5, 0.0), ("b", (3, 4, 5, 7), torch.float32, 3.0, 0.5),
         ("c", (1, 4, 9, 9), torch.float32, 12.0, -1.0), ("d", (2, 4, 8, 8), torch.float16, 7.5, 0.0),
         ("e", (3, 4, 6, 10), torch.float16, 5.0, 0.25))


def extract(path, name):
    tree = ast.parse(open(path).read(), path)
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(body) == 1, name
    ns = {"torch": torch, "__name__": "reference_host_functions"}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns[name]


def main():
    fn = extract(PIPE, "rescale_noise_cfg")
    out = {"phis": np.asarray(PHIS, dtype=np.float64), "cases": np.asarray([c[0] for c in CASES])}
    g = torch.Generator().manual_seed(20231)
    for name, shape, dtype, scale, offset in CASES:
        uncond = torch.randn(shape, generator=g)
        text = (torch.randn(shape, generator=g) * 0.8 + offset)
        uncond, text = uncond.to(dtype), text.to(dtype)
        cfg = uncond + scale * (text - uncond)              # what the denoise loop hands the function
        out[f"{name}_cfg"] = cfg.numpy()
        out[f"{name}_text"] = text.numpy()
        for k, phi in enumerate(PHIS):
            res = fn(cfg, text, guidance_rescale=phi)
            assert res.dtype == dtype and res.shape == cfg.shape
            out[f"{name}_out{k}"] = res.numpy()
    np.savez_compressed(os.path.join(HERE, "guidance_rescale.npz"), **out)
    print("wrote guidance_rescale.npz", {k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main()
