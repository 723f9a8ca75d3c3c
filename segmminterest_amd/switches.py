"""The host-side switches, in one table (the twin of the C library's knob table: ``segmm_config_dump`` / ``segmm_config_set``).

One row per ``SEGMM_*`` environment variable the Python host honours: who reads it, the attribute it becomes on that object,
its default (as the environment would spell it) and its parser.  ``read(owner)`` reads the environment at the moment of the
call -- a ParamStore ("engine"), Trainer ("trainer") or DPComm ("comm") calls it once, in its constructor -- and ``dump()``
lists every row.  Outside this table the package reads SEGMM_LIB and SEGMM_GEMM (hipabi: what is loaded, before any store
exists) and nothing else.  Standard library only: no torch import.
"""
import os
from typing import Callable, NamedTuple, Tuple


class Switch(NamedTuple):
    owners: Tuple[str, ...]      # "engine" (ParamStore), "trainer" (Trainer), "comm" (DPComm)
    attr: str                    # key of read()'s result
    env: str
    default: str                 # spelled as in the environment
    parse: Callable
    doc: str


def flag(s):
    return s != "0"


def tri(s):
    """auto | 0 | 1 -> None | False | True."""
    return None if s == "auto" else s != "0"


def _row(owners, attr, env, default, parse, doc):
    return Switch(tuple(owners.split("+")), attr, "SEGMM_" + env, default, parse, doc)


TABLE = (
    # ---- schedule of the step (streams); none of these changes a result bit
    _row("engine", "overlap", "OVERLAP", "1", flag, "weight/bias gradients and the user-token chains on the side stream (0: one stream)"),
    _row("engine", "defer_wgrad", "DEFER_WGRAD", "auto", tri,
         "a layer's ff/MLP weight gradients enqueued right before its attention backward; auto = S > 32 on the plane engine"),
    _row("engine", "ln_side", "LN_SIDE", "auto", tri, "LayerNorm-backward column sums on the side stream; auto = S > 32 on the plane engine"),
    _row("engine", "lazy_head_grad", "LAZY_HEAD_GRAD", "1", flag, "head gradient formed inside the first LayerNorm backward (trainer's step)"),
    _row("engine", "head_dot", "HEAD_DOT", "1", flag, "Linear(d, 1) head's logits formed inside the last LayerNorm forward"),
    _row("engine+trainer", "side_priority", "SIDE_PRIORITY", "1", int, "priority of the side, auxiliary and prefetch streams (1 = lowest)"),
    # ---- plane protocol of the plane engine (f16x3p)
    _row("engine", "attn_planes_only", "ATTN_PLANES_ONLY", "1", int,
         "attention gradients dQ/dK/dV as planes only + repair pass: 0 off, 1 for S > 32, 2 for every shape"),
    _row("engine", "attn_pl", "ATT_PL", "1", int,
         "attention reads the projection GEMMs' Q/K/V planes: 0 off, 1 planes only, 2 planes beside fp32 (forward only)"),
    _row("engine", "eu_planes_only", "EU_PLANES_ONLY", "1", flag, "user embedding written as planes only (N = 2, trainer's step)"),
    _row("engine", "input_planes_only", "INPUT_PLANES_ONLY", "1", flag, "L1-normalised input features written as planes only"),
    _row("engine", "scaling", "SCALING", "delayed", str,
         "plane scales: delayed (training passes) | exact (split pass after every producer) | always (delayed in evaluation too)"),
    _row("engine", "scale_target", "SCALE_TARGET", "7", int,
         "delayed scales put the last pass's maximum at 2^target (window 2^-2 .. 2^16: 7 leaves 256x of headroom)"),
    _row("engine", "loss_relative", "LOSS_RELATIVE", "1", flag, "backward sites: scale predicted from the site's gain x this step's max |dloss/dlogits|"),
    # ---- the non-plane GEMM engines (f32, bf16x6, on-the-fly f16x3)
    _row("engine", "planes", "PLANES", "1", flag, "bf16x6 / f16x3: pre-split planes of the weights, refreshed once per optimizer step"),
    _row("engine", "wgrad_planes", "WGRAD", "x6", lambda s: 2 if s == "x3" else 3, "bf16x6 weight gradients: x6 (three planes) | x3 (two, opt-in)"),
    _row("engine", "gemm_bn", "GEMM_BN", "", str, "f16x3 tile width forced to 128 | 256 (mirrors the library's choice in the split-K factor)"),
    _row("engine", "split_target", "SPLIT_TARGET", "1024", int, "workgroups a split-K weight gradient aims for"),
    _row("engine", "split_target_p", "SPLIT_TARGET_P", "256", int, "... a plane-operand weight gradient (256 x 256 tiles: the 256 CUs once)"),
    _row("engine", "split_target_few", "SPLIT_TARGET_FEW", "256", int, "... a few-tile plane weight gradient (<= 9 tiles, both widths >= 768)"),
    # ---- trainer and data parallelism
    _row("trainer", "sparse_tables", "SPARSE_TABLES", "1", flag, "data-parallel id tables travel as B rows per rank (0: dense all-reduce)"),
    _row("trainer", "per_bucket_adamw", "BUCKET_ADAMW", "1", flag, "AdamW of a bucket as soon as its all-reduce has landed"),
    _row("trainer", "table_two_pass", "TABLE_TWO_PASS", "1", flag, "id-table AdamW in two passes: untouched rows early, on the auxiliary stream"),
    _row("trainer", "begin_overlap", "BEGIN_OVERLAP", "1", flag, "head of the step (zero_grad, input stage) on two streams"),
    _row("trainer", "bucket_mb", "DP_BUCKET_MB", "8", float, "gradient buckets are merged up to this many MiB per all-reduce"),
    _row("comm", "force", "DP_FORCE", "0", lambda s: s == "1", "1: a one-rank process group still issues every collective (tests)"),
)

RETIRED = {
    "SEGMM_ATTN_FUSED": "the fused dQ+dK+dV attention backward is the only schedule left",
    "SEGMM_ATTN_SPLIT": "dQ on a third stream measured -0.9 % and cannot be recorded; removed",
    "SEGMM_ATTN_TWO_STREAMS": "key blocks on two streams: an A/B arm nothing ran; removed",
    "SEGMM_FEW_TILES": "0 since the 256 x 128 plane tiles: the on-the-fly detour of the plane engine is gone",
    "SEGMM_LN_POS": "the per-position sums of the embedding LayerNorm backward are unconditional",
    "SEGMM_TAIL_BALANCE": "the video-side embedding weight gradient always runs on the main stream",
    "SEGMM_HEAD_SIDE": "the head's weight/bias gradients always run on the side stream (SEGMM_OVERLAP=0: one stream)",
    "SEGMM_USR_SIDE": "a full layer's user-token chain always runs on the side stream (SEGMM_OVERLAP=0: one stream)",
    "SEGMM_FWD_SIDE": "the forward's user-token chain is on the side stream on the plane engine, nowhere else",
}


def _raw(sw):
    return os.environ.get(sw.env, sw.default)


def read(owner):
    """{attribute: parsed value} of ``owner``'s switches, from the environment as it is NOW."""
    for name, why in RETIRED.items():
        if name in os.environ:
            raise RuntimeError("%s is set, but the switch is retired: %s" % (name, why))
    return {sw.attr: sw.parse(_raw(sw)) for sw in TABLE if owner in sw.owners}


def dump():
    """Every row as ``SEGMM_NAME=value  # doc`` (value: what read() would parse now)."""
    return "\n".join("%s=%s  # %s" % (sw.env, _raw(sw), sw.doc) for sw in TABLE)


def launcher_rank():
    """RANK as the launcher exported it (0 without one): mixed into the dropout seed of data-parallel replicas."""
    return int(os.environ.get("RANK", "0"))
