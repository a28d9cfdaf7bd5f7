"""go2netspectra_amd -- MI355X-native sketch hot path for Go2NetSpectra.

Drop-in for the reference's per-packet sketch path (internal/engine/impl/sketch):
header parse -> flow-key encode -> d seeded MurmurHash3 -> fingerprinted
Count-Min / SuperSpread bucket updates, plus the exact per-flow aggregator
(internal/engine/impl/exact), executed by hand-written gfx950 HIP kernels
behind the C ABI in include/gns_sketch.h (libgns_sketch.so).
"""
from . import checkpoint
from ._lib import GnsError, build, load
from .config import Config, ExactTaskDef, SketchTaskDef, load_config, parse_config
from .exact import (Change, ExactAggregator, ExactHistory, ExactTask, ExactView, FlowLifecycle, HeavyHitter, NewExact, SnapshotData, Summary,
                    TaskSummary, apply_delta, discount_heavy_prefixes, make_filter, make_prefix, mask_keys, mask_prefix,
                    merge_summaries, prefix_plan, rollup_plan, signed, spread_rollup_plan, to16_to_encodeflow)
from .factory import Manager, TaskGroup, create, register_aggregator
from .heavy_history import HeavyHistory
from .packets import (CompactBatch, HeaderBatch, PacketBatch, SyntheticTraffic, compact_headers, ip_slot, read_pcap,
                      read_pcap_compact, write_pcap, write_pcapgen, write_pcapng)
from .sketch import CountMin, CountMinView, HeavyCount, HeavyRecord, HeavySize, SuperSpread, SuperSpreadView
from .spread import ExactSpread
from .task import New, SketchTask, decode_flow, encode_flow

__all__ = [
    "GnsError", "build", "load", "Config", "SketchTaskDef", "load_config", "parse_config", "Manager",
    "TaskGroup", "create", "register_aggregator", "HeaderBatch", "PacketBatch", "SyntheticTraffic",
    "ip_slot", "read_pcap", "read_pcap_compact", "compact_headers", "write_pcap", "write_pcapgen", "write_pcapng", "CountMin", "CountMinView", "HeavyCount", "HeavyRecord", "HeavySize",
    "SuperSpread", "New", "SketchTask", "decode_flow", "encode_flow", "ExactTaskDef", "ExactAggregator", "ExactTask",
    "NewExact", "SnapshotData", "ExactSpread", "Summary", "Change", "signed", "TaskSummary", "FlowLifecycle", "HeavyHitter",
    "make_filter", "merge_summaries", "checkpoint", "ExactView", "ExactHistory", "apply_delta", "CompactBatch",
    "SuperSpreadView", "rollup_plan", "spread_rollup_plan", "to16_to_encodeflow",
    "mask_prefix", "mask_keys", "prefix_plan", "make_prefix", "discount_heavy_prefixes", "HeavyHistory",
]
