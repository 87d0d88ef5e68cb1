"""The model of the 16-bit DINO path (test infrastructure; the package never imports it): tests/dino_port.py's network with the two
operands of every matrix product -- patch embedding, qkv, q.k^T, p.v, proj, fc1, fc2 -- rounded once to fp16 / bf16 (to nearest
even) and everything else in fp32: products and sums, the residual stream, LayerNorm, softmax, bias, GELU, the outputs.  `attn` comes
from the fp32 probabilities.  Two placements of the roundings around the softmax, both legitimate for a kernel:

  "A"  the probabilities are normalised in fp32 (exp / row sum), then rounded, then p.v;
  "B"  the flash form: exp(s - m) is rounded, p.v, and the division by the fp32 row sum comes after.

Runs on CPU and GPU tensors alike.  `stats`, if given, collects the largest |operand| seen (what decides whether fp16's range holds).
"""
import torch
import torch.nn.functional as F

import dino_port as port

DEPTH, HEADS, EPS = port.DEPTH, port.HEADS, port.EPS
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
PLACEMENTS = ("A", "B")


def network(sd, img, precision, placement="A", want_blocks=False, stats=None):
    """img: prepared fp32 [B,3,224,224].  Returns dino_port.network's dict, fp32."""
    assert placement in PLACEMENTS, placement
    dt = DTYPES[precision]

    def r(t):
        if stats is not None:
            stats["max_operand"] = max(stats.get("max_operand", 0.0), float(t.abs().max()))
        return t.to(dt).to(torch.float32)

    B = img.shape[0]
    x = F.conv2d(r(img), r(sd["patch_embed.proj.weight"]), sd["patch_embed.proj.bias"], stride=16).flatten(2).transpose(1, 2)
    x = torch.cat((sd["cls_token"].expand(B, -1, -1), x), dim=1)
    x = x + sd["pos_embed"]
    C, N = x.shape[-1], x.shape[1]
    scale = (C // HEADS) ** -0.5
    blocks, attn = [], None
    for i in range(DEPTH):
        p = f"blocks.{i}."
        y = F.layer_norm(x, (C,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], EPS)
        qkv = F.linear(r(y), r(sd[p + "attn.qkv.weight"]), sd[p + "attn.qkv.bias"]).reshape(B, N, 3, HEADS, C // HEADS).permute(2, 0, 3, 1, 4)
        q, k, v = r(qkv[0]), r(qkv[1]), r(qkv[2])
        s = (q @ k.transpose(-2, -1)) * scale
        if placement == "A":
            attn = s.softmax(dim=-1)
            y = r(attn) @ v
        else:
            e = torch.exp(s - s.amax(-1, keepdim=True))
            l = e.sum(-1, keepdim=True)
            attn = e / l
            y = (r(e) @ v) / l
        y = y.transpose(1, 2).reshape(B, N, C)
        x = x + F.linear(r(y), r(sd[p + "attn.proj.weight"]), sd[p + "attn.proj.bias"])
        y = F.layer_norm(x, (C,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], EPS)
        h = F.gelu(F.linear(r(y), r(sd[p + "mlp.fc1.weight"]), sd[p + "mlp.fc1.bias"]))
        x = x + F.linear(r(h), r(sd[p + "mlp.fc2.weight"]), sd[p + "mlp.fc2.bias"])
        if want_blocks:
            blocks.append(x)
    out = {"attn": attn.mean(1).unsqueeze(1)[:, :, 0, 1:], "cls_": x[:, 0, :], "feat": x[:, 1:, :]}
    if want_blocks:
        out["blocks"] = blocks
    return out


def run_case(sd, c, x, precision, placement="A", **kw):
    """Case c of tests/dino_fixture.py on input tensor x (the fixture's input, on any device) with state sd (same device)."""
    with torch.no_grad():
        img = port.prepare(x, c["stride"]) if c["mode"] == "patch" else port.extractor_step2(x)
        return network(sd, img, precision, placement, **kw)
