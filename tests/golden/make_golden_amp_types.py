"""Result types of the REFERENCE's hook modules on fp16 / bf16 feature maps,
with and without the learned soft mask and with per-channel or per-tensor
statistics (CPU, the committed seeded weights).

The amp_*.npz fixtures (make_golden_r06.py) record the default quantizer only
(smooth_transitions=True, per_channel=True).  The inference branch of the
quantizer (_forward_pytorch, quantization.py:729-746) multiplies the
dequantized map by a mask built with F.interpolate(tile_mask.float(), ...)
whether or not the soft mask is on, so the result type does not have to
follow the input; this fixture records what it is for every combination.

Run in the build container only (needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_amp_types.py

Writes tests/golden/amp_types.npz: x (fp16-representable map), x_bf16 (its
bf16-representable copy, as float32), and for every key
<dt>_s<smooth>_c<per_channel> (dt in f16 / bf16, flags 0 / 1):
bits_<key>, y_<key> (the reference's output as float32), dtype_<key> (its dtype
name).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import synth_features  # noqa: E402
from make_golden_r02 import modules  # noqa: E402   (reference analyzer / mapper / quantizer, seeded)

torch.set_num_threads(8)
SHAPE = (2, 16, 20, 20, 8)


def main():
    B, C, H, W, grid = SHAPE
    x = synth_features(B, C, H, W, seed=707008)     # a seed whose tiles take three bit widths (6, 7, 8)
    xb = x.to(torch.bfloat16).float()
    out = dict(B=B, C=C, H=H, W=W, grid=grid, x=x.numpy().astype(np.float16), x_bf16=xb.numpy().astype(np.float32))
    with torch.no_grad():
        for dt, xs in (("f16", x.half()), ("bf16", xb.to(torch.bfloat16))):
            for smooth in (True, False):
                for per_channel in (True, False):
                    a, mapper, q = modules({}, per_channel=per_channel)
                    a.grid_size = grid
                    q.smooth_transitions = smooth
                    key = "%s_s%d_c%d" % (dt, smooth, per_channel)
                    bits = mapper(a(xs), 1.0)
                    y = q(xs, bits, training=False)
                    out["bits_" + key] = bits.numpy()
                    out["y_" + key] = y.float().numpy()
                    out["dtype_" + key] = np.array(str(y.dtype))
                    print(key, "bits", np.unique(out["bits_" + key]).astype(int).tolist(), "y dtype", y.dtype)
    np.savez_compressed(os.path.join(HERE, "amp_types.npz"), **out)


if __name__ == "__main__":
    main()
