"""Standalone decode-attention microbench: kernel time + effective KV
stream rate at the llama-3-8b head config.
Usage: python tools/decode_attn_micro.py [ctx] [B] [--window W]
--window W: sliding-window attention over the last W keys of each context;
the effective rate then counts the keys of the window only."""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from llmapigateway_amd import ops

def run(ctx, B=256, ver=None, window=0):
    dev = "cuda:0"
    Hq, Hkv, BS, D = 32, 8, 64, 128
    maxb = (ctx + BS - 1) // BS
    NB = B * maxb + 8
    kc = torch.randn(NB, Hkv, BS, D, dtype=torch.bfloat16, device=dev)
    vc = torch.randn_like(kc)
    bt = torch.randperm(NB)[: B * maxb].view(B, maxb).int().to(dev)
    q = torch.randn(B, Hq, D, dtype=torch.bfloat16, device=dev)
    lens = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    if ver is not None:
        ops._DECODE_VER = ver
    for _ in range(5):
        ops.attention_decode(q, kc, vc, bt, lens, window=window)
    torch.cuda.synchronize()
    t0 = time.monotonic()
    iters = 200
    for _ in range(iters):
        ops.attention_decode(q, kc, vc, bt, lens, window=window)
    torch.cuda.synchronize()
    us = (time.monotonic() - t0) / iters * 1e6
    keys = min(ctx, window) if window else ctx
    kv_bytes = B * keys * Hkv * D * 2 * 2
    print(f"B={B} ctx={ctx} window={window} v{ops._DECODE_VER}: {us:7.1f} us  "
          f"{kv_bytes/us/1e6:5.2f} TB/s effective")
    return us

if __name__ == "__main__":
    argv = sys.argv[1:]
    window = 0
    if "--window" in argv:
        i = argv.index("--window")
        window = int(argv[i + 1])
        del argv[i : i + 2]
    if argv:
        run(int(argv[0]), int(argv[1]) if len(argv) > 1 else 256, window=window)
    else:
        for v in (2, 3):
            for c in (192, 512, 2048, 8192):
                run(c, ver=v)
