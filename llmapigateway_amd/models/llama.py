"""Llama-family decoder (Llama-3, Mistral) built directly on the MI355X ops.

Inference-only, bf16 weights, random init (no network for checkpoints —
BASELINE.json: synthetic data / random-init weights). The forward pass is a
flat varlen batch (ForwardBatch) in one of two modes:

- prefill: fresh prompts; ops.attention_prefill over the batch's own K/V
  (and K/V written to the paged cache for later decode);
- decode: one token per running sequence; ops.attention_decode over the
  paged cache via block tables.

Projections run through ops.linear: decode-shaped batches (8 < M <= 256)
hit the macro-tile LDS-staged gfx950 GEMM (ops/csrc/gemm_m256.hip) for the
shapes its measured dispatch table wins (o/down; gate_up with the swiglu
fused into the epilogue), the streaming skinny kernel
(ops/csrc/gemm_skinny.hip) serves the M <= 16 latency regime without a
fragment twin, and prefill batches, qkv and lm_head use the TunableOp-tuned
hipBLASLt/rocBLAS library GEMMs. The o- and down-projections also produce
the following RMSNorm (ops.linear_rmsnorm_residual): on the split-K decode
path the slab reduction, residual add and norm are one kernel. The other hot
ops (rope, attention, sampling) are the hand-written CDNA4 kernels behind
llmapigateway_amd.ops.

Multi-LoRA: with ``max_loras > 0`` the model holds that many adapter slots
per layer and projection (ops.LoraStack) and adds ``ForwardBatch.adapter_ids``'
per-row delta after each projection GEMM (ops.lora_add, ops/csrc/lora.hip);
o/down then run linear + delta + rmsnorm_residual and gate_up linear + delta
+ swiglu, not the fused ops (see forward()).

Tensor parallelism: construct with ``tp_group`` + a config pre-sharded via
ModelConfig.scaled_for_tp; qkv/gate_up are column-sharded, o/down
row-sharded with an RCCL all-reduce over xGMI after each (2 per layer).
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch
import torch.distributed as dist
import torch.nn.functional as F

from .. import ops
from .configs import ModelConfig


@dataclass
class ForwardBatch:
    kind: str  # "prefill" | "decode" | "mixed"
    token_ids: torch.Tensor          # [T] int64
    positions: torch.Tensor          # [T] int64
    slot_mapping: torch.Tensor       # [T] int64 (global KV slots; -1 = don't write)
    # prefill:
    cu_seqlens: Optional[torch.Tensor] = None   # [B+1] int32
    max_seqlen: int = 0
    tile_seq: Optional[torch.Tensor] = None     # [ntiles] int32 (GPU kernel tile map)
    tile_off: Optional[torch.Tensor] = None
    # decode:
    block_tables: Optional[torch.Tensor] = None  # [B, max_blocks] int32
    context_lens: Optional[torch.Tensor] = None  # [B] int32
    # prefill with cached prefix (prefix caching): per-seq number of
    # positions already in the paged cache (block_tables set too)
    cached_lens: Optional[torch.Tensor] = None   # [B] int32
    # rows of the flat batch at which logits are needed (last token per seq)
    logits_indices: Optional[torch.Tensor] = None  # [B] int64
    # mixed steps: rows [0, n_prefill_tokens) are prefill (cu_seqlens etc.
    # apply to them), rows [n_prefill_tokens, T) are decode rows with their
    # own tables/lens (decode never shares block_tables with the cached-
    # prefill phase in a mixed step)
    n_prefill_tokens: int = 0
    dec_block_tables: Optional[torch.Tensor] = None  # [Bd, max_blocks] int32
    dec_context_lens: Optional[torch.Tensor] = None  # [Bd] int32
    # multi-LoRA: adapter slot of every row of the flat batch (-1 = base
    # model); None = all base. Read only by a model built with max_loras > 0
    adapter_ids: Optional[torch.Tensor] = None       # [T] int32


class LlamaModel:
    def __init__(
        self,
        config: ModelConfig,
        device: torch.device | str = "cpu",
        dtype: torch.dtype = torch.bfloat16,
        seed: int = 0,
        tp_group: Optional[object] = None,
        tp_rank: int = 0,
        tp_size: int = 1,
        full_config: Optional[ModelConfig] = None,
        weight_dtype: str = "auto",
        max_loras: int = 0,
        max_lora_rank: int = 16,
    ):
        if weight_dtype not in ("auto", "fp8", "mxfp4"):
            raise ValueError(
                f"weight_dtype must be 'auto', 'fp8' or 'mxfp4', got {weight_dtype!r}"
            )
        # "fp8": the four projections of every layer are held as e4m3 bits
        # (fragment-major, ops.swizzle_weight_frag_fp8) plus one fp32 scale
        # per output channel, and run through ops.linear_w8; embeddings,
        # lm_head and norms stay in `dtype`.
        # "mxfp4": the same four as OCP MXFP4 — e2m1 nibbles plus one e8m0
        # scale per 32 k of a row (fragment-major,
        # ops.swizzle_weight_frag_mxfp4) — run through ops.linear_w4
        self.weight_dtype = weight_dtype
        self.config = config
        self.full_config = full_config or config
        self.device = torch.device(device)
        self.dtype = dtype
        self.tp_group = tp_group
        self.tp_rank = tp_rank
        self.tp_size = tp_size
        self.scale = config.head_dim ** -0.5
        # sliding-window attention: a constant of the model (0 = none),
        # so captured decode graphs stay valid
        self.window = int(config.sliding_window or 0)
        self.layers: List[Dict[str, torch.Tensor]] = []
        # multi-LoRA: max_loras adapter slots resident next to the base
        # weights (0 = none: nothing is allocated and forward() is the
        # adapter-free code). Set before the weights: _build_twins reads it
        self.max_loras = int(max_loras)
        self._init_weights(seed)
        self.lora_layers: List[Dict[str, "ops.LoraStack"]] = []
        if self.max_loras < 0:
            raise ValueError(f"max_loras must be >= 0, got {max_loras}")
        if self.max_loras:
            if tp_size > 1:
                raise NotImplementedError(
                    "LoRA adapters (max_loras > 0) are not supported with "
                    "tensor parallelism (tp_size > 1) yet"
                )
            self._init_lora_stacks(int(max_lora_rank))
        self.cos_sin = ops.build_rope_cache(
            config.max_positions, config.head_dim, config.rope_theta, device=self.device
        )

    # ---- weights ----
    def _init_weights(self, seed: int) -> None:
        c = self.config
        hidden = c.hidden_size
        # tiny models init on CPU (deterministic across devices, for tests);
        # big models init directly on the GPU (CPU RNG would take minutes at 8B+)
        approx_params = (
            2 * self.full_config.vocab_size * hidden
            + c.num_layers * hidden * (c.q_size + 2 * c.kv_size + c.q_size + 3 * c.intermediate_size) // 1
        )
        init_device = torch.device("cpu") if approx_params < 10**8 else self.device
        gen = torch.Generator(device=init_device).manual_seed(seed)

        def mk(rows: int, cols: int, std: float) -> torch.Tensor:
            w = torch.empty(rows, cols, dtype=torch.float32, device=init_device)
            w.normal_(0.0, std, generator=gen)
            return w.to(self.dtype).to(self.device)

        # TP: every rank draws the same full-shape weights (same seed) and
        # keeps its Megatron-style slice (parallel/tp.py), so TP=N is a pure
        # sharding of the TP=1 model (gloo CPU test asserts logits parity).
        from ..parallel.tp import shard_column, shard_gate_up, shard_qkv, shard_row

        fc = self.full_config
        tpr, tps = self.tp_rank, self.tp_size

        std = 0.02
        out_std = 0.02 / math.sqrt(2 * c.num_layers)
        self.embed = mk(fc.vocab_size, hidden, std)
        quant = self.weight_dtype != "auto"
        for _ in range(c.num_layers):
            qkv_full = mk(fc.q_size + 2 * fc.kv_size, hidden, std)
            o_full = mk(hidden, fc.q_size, out_std)
            gu_full = mk(2 * fc.intermediate_size, hidden, std)
            down_full = mk(hidden, fc.intermediate_size, out_std)
            if quant:
                # quantise the FULL matrices layer by layer (peak memory
                # stays near the quantised size), then shard bits and scales:
                # TP=N stays a pure sharding of the TP=1 quantised model
                self.layers.append(
                    self._quant_layer(qkv_full, o_full, gu_full, down_full)
                )
                del qkv_full, o_full, gu_full, down_full
                continue
            self.layers.append(
                {
                    "input_norm": torch.ones(hidden, dtype=self.dtype, device=self.device),
                    "qkv": shard_qkv(qkv_full, tpr, tps, fc.q_size, fc.kv_size)
                    if tps > 1
                    else qkv_full,
                    "o": shard_row(o_full, tpr, tps) if tps > 1 else o_full,
                    "post_norm": torch.ones(hidden, dtype=self.dtype, device=self.device),
                    "gate_up": shard_gate_up(gu_full, tpr, tps, fc.intermediate_size)
                    if tps > 1
                    else gu_full,
                    "down": shard_row(down_full, tpr, tps) if tps > 1 else down_full,
                }
            )
        self.final_norm = torch.ones(hidden, dtype=self.dtype, device=self.device)
        self.lm_head = self.embed if c.tie_embeddings else mk(self.full_config.vocab_size, hidden, std)

        if quant:
            self._reserve_w8_buffer()
            return  # no bf16 matrices, so no bf16 twins
        self._build_twins()

    def _quant_layer(self, qkv_full, o_full, gu_full, down_full) -> Dict[str, torch.Tensor]:
        """One layer's dict in a quantised mode, from the full (unsharded)
        matrices. fp8: `<name>_q8` (fragment-major e4m3 bits) and `<name>_s8`
        (fp32 scale per output channel) for the four projections. mxfp4:
        `<name>_q4` (fragment-major e2m1 nibbles) and `<name>_s4`
        (fragment-major e8m0 block scales)."""
        from ..parallel.tp import shard_gate_up, shard_qkv, shard_row

        fc, tpr, tps = self.full_config, self.tp_rank, self.tp_size
        hidden = self.config.hidden_size
        layer: Dict[str, torch.Tensor] = {
            "input_norm": torch.ones(hidden, dtype=self.dtype, device=self.device),
            "post_norm": torch.ones(hidden, dtype=self.dtype, device=self.device),
        }
        for name, full in (
            ("qkv", qkv_full), ("o", o_full), ("gate_up", gu_full), ("down", down_full)
        ):
            mx = self.weight_dtype == "mxfp4"
            q, s = (ops.mxfp4_quantize_weight if mx else ops.fp8_quantize_weight)(full)
            if tps > 1:
                if name == "qkv":
                    q = shard_qkv(q, tpr, tps, fc.q_size, fc.kv_size)
                    s = shard_qkv(s, tpr, tps, fc.q_size, fc.kv_size)
                elif name == "gate_up":
                    q = shard_gate_up(q, tpr, tps, fc.intermediate_size)
                    s = shard_gate_up(s, tpr, tps, fc.intermediate_size)
                else:  # row-parallel: every rank keeps all output channels
                    q = shard_row(q, tpr, tps)
                    if mx:  # K-shards are multiples of 64: whole blocks
                        s = shard_row(s, tpr, tps)
            (self._store_w4 if mx else self._store_w8)(layer, name, q, s)
        return layer

    @staticmethod
    def _store_w8(layer, name: str, q: torch.Tensor, s: torch.Tensor) -> None:
        if q.shape[0] % 64 or q.shape[1] % 64:
            raise ValueError(
                f"fp8 weights need projection shapes in multiples of 64; "
                f"{name} is {tuple(q.shape)}"
            )
        layer[name + "_q8"] = ops.swizzle_weight_frag_fp8(q)
        layer[name + "_s8"] = s.contiguous()

    @staticmethod
    def _store_w4(layer, name: str, packed: torch.Tensor, s: torch.Tensor) -> None:
        if packed.shape[0] % 64 or (packed.shape[1] * 2) % 64:
            raise ValueError(
                f"mxfp4 weights need projection shapes in multiples of 64; "
                f"{name} is {(packed.shape[0], packed.shape[1] * 2)}"
            )
        layer[name + "_q4"], layer[name + "_s4"] = ops.swizzle_weight_frag_mxfp4(
            packed, s
        )

    def _reserve_w8_buffer(self) -> None:
        """The M > 256 route dequantises into one per-device bf16 buffer:
        size it for the largest projection now, so captured graphs never
        see it move."""
        if self.device.type != "cuda":
            return
        # hand the quantiser's temporaries (full bf16 matrices, fp32 copies)
        # back to the device first: the KV pool is sized from free memory
        torch.cuda.empty_cache()
        key, per_byte = ("_q4", 2) if self.weight_dtype == "mxfp4" else ("_q8", 1)
        ops.w8_reserve_dequant(
            self.device,
            max(
                layer[name + key].numel() * per_byte
                for layer in self.layers
                for name in ("qkv", "o", "gate_up", "down")
            ),
        )

    @torch.inference_mode()
    def quantize_weights_(self, mode: str = "fp8", simulate: bool = False) -> "LlamaModel":
        """Quantise the qkv/o/gate_up/down projections of a bf16 model in
        place; mode is "fp8" or "mxfp4". simulate=False leaves the model as
        weight_dtype=mode builds it (twin + scales only). simulate=True is
        fake-quant: every
        projection becomes its dequantised value in the model dtype and the
        bf16 twins are rebuilt — the same maths on the existing kernels, as
        an oracle and an accuracy A/B."""
        if mode not in ("fp8", "mxfp4"):
            raise ValueError(f"unknown quantisation mode {mode!r}")
        if self.weight_dtype != "auto":
            raise RuntimeError(f"weights are already {self.weight_dtype}")
        if self.tp_size > 1:
            # row shards would get per-shard scales: not the TP=1 model
            raise RuntimeError(
                "quantize_weights_ works on an unsharded model; under tensor "
                f"parallelism construct with weight_dtype={mode!r}"
            )
        names = ("qkv", "o", "gate_up", "down")
        if mode == "mxfp4":
            quantize, dequantize, store = (
                ops.mxfp4_quantize_weight, ops.mxfp4_dequantize_weight, self._store_w4
            )
        else:
            quantize, dequantize, store = (
                ops.fp8_quantize_weight, ops.fp8_dequantize_weight, self._store_w8
            )
        for layer in self.layers:
            for key in [k for k in layer if k.endswith(("_swz", "_int"))]:
                del layer[key]
            for name in names:
                q, s = quantize(layer[name])
                if simulate:
                    layer[name] = dequantize(q, s, self.dtype)
                else:
                    del layer[name]
                    store(layer, name, q, s)
        if simulate:
            self._build_twins()
        else:
            self.weight_dtype = mode
            self._reserve_w8_buffer()
        return self

    def _build_twins(self) -> None:
        # Fragment-major twins of the decode projections for the
        # macro-tile LDS-staged GEMM (ops/csrc/gemm_m256.hip) — ON by
        # default: the twin copy costs ~weights-again for the projections
        # (~14 GB for llama-3-8b, cheap against 288 GB HBM) and buys the
        # decode step its dominant GEMM time back from the library
        # (profiles/r02_gemm_m256_probe.md). LLMAPI_NO_FRAG_WEIGHTS=1
        # opts out; LLMAPI_SWZ_WEIGHTS=1 selects the legacy k-major twins
        # (gemm_skinny streaming form) for comparison runs.
        import os as _os

        if self.device.type == "cuda" and not _os.environ.get("LLMAPI_NO_FRAG_WEIGHTS"):
            legacy = bool(_os.environ.get("LLMAPI_SWZ_WEIGHTS"))
            for layer in self.layers:
                for name in ("qkv", "o", "gate_up", "down"):
                    w = layer[name]
                    if legacy:
                        if w.shape[0] % 64 == 0 and w.shape[1] % 32 == 0:
                            layer[name + "_swz"] = ops.swizzle_weight(w)
                    elif (
                        w.shape[0] % 64 == 0
                        and w.shape[1] % 64 == 0
                        # only shapes the measured dispatch actually routes to
                        # the custom kernel get a twin — qkv/gate_up twins
                        # would be dead HBM (the library wins those shapes),
                        # ~9 GB at 8B and ~89 GB at 70B
                        and ops._m256_config(256, w.shape[0], w.shape[1]) is not None
                        # gate_up with a fused-swiglu twin never uses the
                        # plain twin — don't hold both in HBM
                        and not (
                            name == "gate_up"
                            and not getattr(self, "max_loras", 0)
                            and ops._m256_swiglu_config(
                                256, w.shape[0], w.shape[1]
                            )
                            is not None
                        )
                    ):
                        layer[name + "_swz"] = ops.swizzle_weight_frag(w)
                gu = layer["gate_up"]
                if (
                    not legacy
                    # with adapters resident gate_up never takes the fused
                    # swiglu route (forward()): its twin would be dead HBM
                    and not getattr(self, "max_loras", 0)
                    and ops._m256_swiglu_config(256, gu.shape[0], gu.shape[1])
                    is not None
                ):
                    # block-16 interleaved twin for the FUSED gate_up+swiglu
                    # decode path (ops.swiglu_linear)
                    layer["gate_up_int"] = ops.swizzle_weight_frag(
                        ops.interleave_gate_up(gu)
                    )

    # ---- LoRA adapters ----
    # PEFT target -> (fused projection, segment within it)
    LORA_TARGETS = {
        "q_proj": ("qkv", 0), "k_proj": ("qkv", 1), "v_proj": ("qkv", 2),
        "o_proj": ("o", 0), "gate_proj": ("gate_up", 0),
        "up_proj": ("gate_up", 1), "down_proj": ("down", 0),
    }

    def _lora_shapes(self) -> Dict[str, tuple]:
        """projection -> (K, segment widths). gate_up is [gate; up] stacked:
        with adapters resident it always takes the plain linear route."""
        c = self.config
        return {
            "qkv": (c.hidden_size, (c.q_size, c.kv_size, c.kv_size)),
            "o": (c.q_size, (c.hidden_size,)),
            "gate_up": (c.hidden_size, (c.intermediate_size, c.intermediate_size)),
            "down": (c.intermediate_size, (c.hidden_size,)),
        }

    def _init_lora_stacks(self, max_rank: int) -> None:
        """Slot stacks for every layer and projection, allocated once (a
        captured decode graph holds their addresses) and zero: an empty slot
        adds nothing. Per slot: true rank (the kernels stop there) and
        alpha / r, shared by all stacks."""
        S, R = self.max_loras, ops.lora_padded_rank(max_rank)
        self.max_lora_rank = R
        dev = self.device
        self.lora_ranks = torch.zeros(S, dtype=torch.int32, device=dev)
        self.lora_scales = torch.zeros(S, dtype=torch.float32, device=dev)
        for _ in self.layers:
            stacks = {}
            for name, (K, widths) in self._lora_shapes().items():
                bounds = [sum(widths[: i + 1]) for i in range(len(widths))]
                stacks[name] = ops.LoraStack(
                    torch.zeros(S, len(widths) * R, K, dtype=self.dtype, device=dev),
                    torch.zeros(S, bounds[-1], R, dtype=self.dtype, device=dev),
                    self.lora_ranks, self.lora_scales, bounds,
                )
            self.lora_layers.append(stacks)

    def lora_bytes(self) -> int:
        return sum(
            t.numel() * t.element_size()
            for stacks in self.lora_layers
            for st in stacks.values()
            for t in (st.A, st.B)
        )

    @torch.inference_mode()
    def set_adapter(
        self, slot: int, tensors: Dict[str, torch.Tensor],
        alpha: Optional[float] = None,
    ) -> int:
        """Pack one adapter into slot `slot` of every stack, in place.
        `tensors` is PEFT-style: "layers.<i>.<target>.lora_A" [r, K] and
        "layers.<i>.<target>.lora_B" [N_part, r] for target in q_proj,
        k_proj, v_proj, o_proj, gate_proj, up_proj, down_proj; a missing
        target contributes zero. The fused projections stack their targets'
        A along the segment axis and B along the output columns. alpha
        defaults to r (scale 1). Returns r."""
        if not (0 <= slot < self.max_loras):
            raise ValueError(f"adapter slot {slot} outside [0, {self.max_loras})")
        ranks = {t.shape[0] for k, t in tensors.items() if k.endswith(".lora_A")}
        if len(ranks) != 1:
            raise ValueError(f"an adapter needs one rank for all targets, got {sorted(ranks)}")
        r = ranks.pop()
        R = self.max_lora_rank
        if not (1 <= r <= R):
            raise ValueError(f"adapter rank {r} outside [1, max_lora_rank={R}]")
        known = set()
        shapes = self._lora_shapes()
        for i, stacks in enumerate(self.lora_layers):
            for st in stacks.values():
                st.A[slot].zero_()
                st.B[slot].zero_()
            for target, (name, seg) in self.LORA_TARGETS.items():
                ka, kb = (f"layers.{i}.{target}.lora_{x}" for x in "AB")
                if ka not in tensors and kb not in tensors:
                    continue
                known.update((ka, kb))
                a, b = tensors[ka], tensors[kb]
                K, widths = shapes[name]
                lo = sum(widths[:seg])
                if tuple(a.shape) != (r, K) or tuple(b.shape) != (widths[seg], r):
                    raise ValueError(
                        f"layers.{i}.{target}: expected lora_A {(r, K)} and "
                        f"lora_B {(widths[seg], r)}, got {tuple(a.shape)} and "
                        f"{tuple(b.shape)}"
                    )
                st = stacks[name]
                st.A[slot, seg * R : seg * R + r].copy_(a)
                st.B[slot, lo : lo + widths[seg], :r].copy_(b)
        unknown = set(tensors) - known
        if unknown:
            raise ValueError(f"unknown adapter tensors: {sorted(unknown)[:4]}")
        self.lora_ranks[slot] = r
        self.lora_scales[slot] = float(alpha if alpha is not None else r) / r
        return r

    def clear_adapter(self, slot: int) -> None:
        """Empty a slot: rank 0, so its rows add nothing."""
        self.lora_ranks[slot] = 0
        self.lora_scales[slot] = 0.0

    def random_adapter(
        self, rank: int, seed: int = 0, targets: Optional[List[str]] = None
    ) -> Dict[str, torch.Tensor]:
        """A seeded synthetic adapter in set_adapter's layout (the base model
        is random-init too). Both factors are N(0, 0.02), lora_B included,
        so the adapter moves the logits visibly."""
        targets = list(self.LORA_TARGETS) if targets is None else list(targets)
        bad = [t for t in targets if t not in self.LORA_TARGETS]
        if bad:
            raise ValueError(f"unknown LoRA targets {bad}")
        gen = torch.Generator().manual_seed(seed)
        shapes = self._lora_shapes()
        out: Dict[str, torch.Tensor] = {}
        for i in range(len(self.layers)):
            for target in targets:
                name, seg = self.LORA_TARGETS[target]
                K, widths = shapes[name]
                out[f"layers.{i}.{target}.lora_A"] = torch.empty(rank, K).normal_(
                    0.0, 0.02, generator=gen)
                out[f"layers.{i}.{target}.lora_B"] = torch.empty(
                    widths[seg], rank).normal_(0.0, 0.02, generator=gen)
        return out

    def _linear_lora(self, x, layer, name: str, stacks, adapter_ids) -> torch.Tensor:
        """Base projection, then the per-row adapter delta on its bf16
        output: the same on every weight_dtype route."""
        y = self._linear(x, layer, name)
        return ops.lora_add(y, x, stacks[name], adapter_ids)

    def param_bytes(self) -> int:
        tensors = [self.embed, self.final_norm]
        if self.lm_head is not self.embed:
            tensors.append(self.lm_head)
        for layer in self.layers:
            tensors.extend(layer.values())
        return sum(t.numel() * t.element_size() for t in tensors)

    # ---- forward ----
    def _maybe_all_reduce(self, x: torch.Tensor) -> torch.Tensor:
        if self.tp_group is not None:
            dist.all_reduce(x, group=self.tp_group)
        return x

    def _linear(self, x: torch.Tensor, layer, name: str) -> torch.Tensor:
        if self.weight_dtype == "fp8":
            return ops.linear_w8(x, layer[name + "_q8"], layer[name + "_s8"])
        if self.weight_dtype == "mxfp4":
            return ops.linear_w4(x, layer[name + "_q4"], layer[name + "_s4"])
        return ops.linear(x, layer[name], layer.get(name + "_swz"))

    def _row_parallel(self, x: torch.Tensor, layer, name: str) -> torch.Tensor:
        """Row-parallel linear with comm/compute overlap: split the token
        batch in two, launch the first half's all-reduce asynchronously
        while the second half's GEMM runs (overlap the 2
        all-reduces/layer with compute). Falls back to the plain form for
        tiny batches or TP=1."""
        if self.tp_group is None:
            return self._linear(x, layer, name)
        T = x.shape[0]
        if T < 32:  # split overhead exceeds the overlap win
            y = self._linear(x, layer, name)
            dist.all_reduce(y, group=self.tp_group)
            return y
        half = T // 2
        y1 = self._linear(x[:half], layer, name)
        h1 = dist.all_reduce(y1, group=self.tp_group, async_op=True)
        y2 = self._linear(x[half:], layer, name)
        h2 = dist.all_reduce(y2, group=self.tp_group, async_op=True)
        h1.wait()
        h2.wait()
        return torch.cat([y1, y2], dim=0)

    def _row_parallel_norm(self, x, layer, name, residual, norm_w):
        """Row-parallel linear followed by the residual-add RMSNorm ->
        (normed, residual). Without TP the two go through one op so the
        decode path can fuse the norm into the split-K reduction; under TP
        the all-reduce sits between GEMM and norm, so they stay separate."""
        eps = self.config.rms_eps
        if self.tp_group is None:
            if self.weight_dtype == "fp8":
                return ops.linear_w8_rmsnorm_residual(
                    x, layer[name + "_q8"], layer[name + "_s8"], residual,
                    norm_w, eps,
                )
            if self.weight_dtype == "mxfp4":
                return ops.linear_w4_rmsnorm_residual(
                    x, layer[name + "_q4"], layer[name + "_s4"], residual,
                    norm_w, eps,
                )
            return ops.linear_rmsnorm_residual(
                x, layer[name], layer.get(name + "_swz"), residual, norm_w, eps
            )
        return ops.rmsnorm_residual(
            self._row_parallel(x, layer, name), residual, norm_w, eps
        )

    @torch.inference_mode()
    def forward(
        self,
        batch: ForwardBatch,
        k_caches: List[torch.Tensor],
        v_caches: List[torch.Tensor],
        k_scales: "Optional[List[torch.Tensor]]" = None,
        v_scales: "Optional[List[torch.Tensor]]" = None,
    ) -> torch.Tensor:
        """Returns logits [B, vocab] at batch.logits_indices. With
        k_scales/v_scales the caches are fp8 e4m3 (per-row scales).

        A model built with max_loras > 0 adds batch.adapter_ids' adapter
        delta after each of the four projection GEMMs (ops.lora_add), and
        then o and down run linear + delta + ops.rmsnorm_residual instead
        of the fused GEMM+norm op, and gate_up runs linear + delta +
        ops.swiglu instead of the fused swiglu GEMM: the price of adapters
        being resident, paid by base rows too
        (profiles/r10_multi_lora.md)."""
        c = self.config
        stacks_all = self.lora_layers if self.max_loras else None
        aid = None
        if stacks_all is not None:
            aid = batch.adapter_ids
            if aid is None:
                aid = torch.full(
                    (batch.token_ids.shape[0],), -1, dtype=torch.int32,
                    device=self.device,
                )
        ksc = k_scales if k_scales is not None else [None] * len(self.layers)
        vsc = v_scales if v_scales is not None else [None] * len(self.layers)
        h = F.embedding(batch.token_ids, self.embed)
        T = h.shape[0]
        # layer 0 norms the embeddings directly; every later input_norm (and
        # the final norm) comes out of the previous layer's down-projection
        x, residual = ops.rmsnorm(h, self.layers[0]["input_norm"], c.rms_eps), h
        n_layers = len(self.layers)

        for i, layer in enumerate(self.layers):

            lora = stacks_all[i] if stacks_all is not None else None
            if lora is None:
                qkv = self._linear(x, layer, "qkv")
            else:
                qkv = self._linear_lora(x, layer, "qkv", lora, aid)
            q, k, v = qkv.split([c.q_size, c.kv_size, c.kv_size], dim=-1)
            q = q.view(T, c.num_heads, c.head_dim)
            k = k.view(T, c.num_kv_heads, c.head_dim)
            v = v.view(T, c.num_kv_heads, c.head_dim)
            ops.rope_and_kv_write(
                q, k, v, k_caches[i], v_caches[i],
                batch.positions, self.cos_sin, batch.slot_mapping,
                k_scale=ksc[i], v_scale=vsc[i],
            )

            if batch.kind == "prefill":
                attn = ops.attention_prefill(
                    q, k, v, batch.cu_seqlens, batch.max_seqlen, self.scale,
                    tile_seq=batch.tile_seq, tile_off=batch.tile_off,
                    k_cache=k_caches[i] if batch.cached_lens is not None else None,
                    v_cache=v_caches[i] if batch.cached_lens is not None else None,
                    block_tables=batch.block_tables,
                    cached_lens=batch.cached_lens,
                    k_scale=ksc[i] if batch.cached_lens is not None else None,
                    v_scale=vsc[i] if batch.cached_lens is not None else None,
                    window=self.window,
                )
            elif batch.kind == "mixed":
                Tp = batch.n_prefill_tokens
                attn_p = ops.attention_prefill(
                    q[:Tp], k[:Tp], v[:Tp], batch.cu_seqlens, batch.max_seqlen,
                    self.scale, tile_seq=batch.tile_seq, tile_off=batch.tile_off,
                    k_cache=k_caches[i] if batch.cached_lens is not None else None,
                    v_cache=v_caches[i] if batch.cached_lens is not None else None,
                    block_tables=batch.block_tables,
                    cached_lens=batch.cached_lens,
                    k_scale=ksc[i] if batch.cached_lens is not None else None,
                    v_scale=vsc[i] if batch.cached_lens is not None else None,
                    window=self.window,
                )
                attn_d = ops.attention_decode(
                    q[Tp:], k_caches[i], v_caches[i],
                    batch.dec_block_tables, batch.dec_context_lens, self.scale,
                    k_scale=ksc[i], v_scale=vsc[i], window=self.window,
                )
                attn = torch.cat([attn_p, attn_d], dim=0)
            else:
                attn = ops.attention_decode(
                    q, k_caches[i], v_caches[i], batch.block_tables,
                    batch.context_lens, self.scale,
                    k_scale=ksc[i], v_scale=vsc[i], window=self.window,
                )

            next_norm = (
                self.layers[i + 1]["input_norm"] if i + 1 < n_layers
                else self.final_norm
            )
            if lora is not None:
                x, residual = ops.rmsnorm_residual(
                    self._linear_lora(
                        attn.reshape(T, c.q_size), layer, "o", lora, aid
                    ),
                    residual, layer["post_norm"], c.rms_eps,
                )
                act = ops.swiglu(self._linear_lora(x, layer, "gate_up", lora, aid))
                x, residual = ops.rmsnorm_residual(
                    self._linear_lora(act, layer, "down", lora, aid),
                    residual, next_norm, c.rms_eps,
                )
                continue
            x, residual = self._row_parallel_norm(
                attn.reshape(T, c.q_size), layer, "o",
                residual, layer["post_norm"],
            )
            if self.weight_dtype != "auto":
                act = ops.swiglu(self._linear(x, layer, "gate_up"))
            else:
                act = ops.swiglu_linear(
                    x, layer["gate_up"], layer.get("gate_up_swz"),
                    layer.get("gate_up_int"),
                )
            x, residual = self._row_parallel_norm(
                act, layer, "down", residual, next_norm,
            )

        if batch.logits_indices is not None:
            x = x[batch.logits_indices]
        return ops.linear(x, self.lm_head).float()
