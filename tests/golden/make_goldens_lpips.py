"""tests/golden/lpips.npz: the inputs of the LPIPS cases (tests/lpips_weights.CASES), the fp64 port's value and per-layer values,
e32 = |port_fp32 - port_fp64| of both, the feature maps' scales and e32, and the sha256 of each generated state.  Pins the port and
the weight generator against drift.  Run from the repository root: python tests/golden/make_goldens_lpips.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lpips_port as port          # noqa: E402
import lpips_weights as lw         # noqa: E402


def main():
    torch.set_num_threads(8)
    out = {}
    states = {k: lw.make_state(k, lw.STATE_SEEDS[k]) for k in lw.KINDS}
    for k, sd in states.items():
        out[f"sha256_{k}"] = np.array(lw.state_sha256(sd))
    for ci, (name, n, h, w, sigma, kinds) in enumerate(lw.CASES):
        a, b = lw.make_images(ci)
        out[f"{name}_img0"], out[f"{name}_img1"] = a, b
        ta, tb = torch.from_numpy(a), torch.from_numpy(b)
        for kind in kinds:
            v64, l64, f0_64, f1_64 = port.lpips(states[kind], ta, tb, torch.float64)
            v32, l32, f0_32, f1_32 = port.lpips(states[kind], ta, tb, torch.float32)
            key = f"{name}_{kind}"
            out[key + "_value"], out[key + "_layers"] = v64.numpy(), l64.numpy()
            out[key + "_value_e32"] = (v32.double() - v64).abs().numpy()
            out[key + "_layers_e32"] = (l32.double() - l64).abs().numpy()
            out[key + "_feat_scale"] = np.array([max(float(f0_64[l].abs().max()), float(f1_64[l].abs().max())) for l in range(5)])
            out[key + "_feat_e32"] = np.array([max(float((f0_32[l].double() - f0_64[l]).abs().max()),
                                                   float((f1_32[l].double() - f1_64[l]).abs().max())) for l in range(5)])
            share = [max(port.zero_pixel_share(f0_64[l]), port.zero_pixel_share(f1_64[l])) for l in range(5)]
            out[key + "_zero_share"] = np.array(share)
            rel = float(out[key + "_value_e32"].max() / v64.abs().max())
            print(f"{key:18s} value {v64.flatten().tolist()} rel e32 {rel:.2e} zero-pixel share {['%.3f' % s for s in share]}")
            assert 4 * out[key + "_value_e32"].max() <= 1e-4 * float(v64.abs().max()), key
            if kind == "sparse":
                for l in (2, 4):
                    assert 0.0 < share[l] < 1.0, (key, l, share[l])
    path = os.path.join(HERE, "lpips.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
