"""rawalign_amd -- MI355X-native DTW alignment engine behind RawAlign's align_chain.

The package holds only what the hot path needs: ``csrc/`` (hand-written gfx950 kernels and the
C ABI of ``include/rawdtw.h``), a ctypes binding to that ABI, and the host-side mirror of the
reference interface for this path (``dtw.hpp`` function names, ``align_chain`` semantics).

There is no CPU fallback: importing works anywhere, but every compute call needs
``librawdtw.so`` and a HIP device and raises otherwise.
"""
from ._lib import LibraryMissing, RawDTWError, load_library, library_path  # noqa: F401
from .dtw import ANCHOR_DTYPE, CHAIN_REC_DTYPE, JOB_DTYPE, RAWDTW_FULL, ROUND_OUT_DTYPE, SEED_DTYPE, DtwResult, Engine, Plan, ALN_REC_DTYPE, aln_text_bound, aln_text_host, banded_tb_host, chain_decline_host, expand_steps, round_end_host, round_keep_host, semiglobal_host, semiglobal_place_reduce, semiglobal_span_host, semiglobal_tb_window_host  # noqa: F401
from .align import (  # noqa: F401
    RI_M_DTW_BORDER_CONSTRAINT_GLOBAL,
    RI_M_DTW_BORDER_CONSTRAINT_SPARSE,
    RI_M_DTW_FILL_METHOD_BANDED,
    RI_M_DTW_FILL_METHOD_FULL,
    Batch,
    CandidateBatch,
    Chain,
    MapOpt,
    ReadCandidates,
    align_chain,
    evaluate_reads,
)

from .events import EventOptions, chunks_of, detect_events, detect_events_host  # noqa: F401
from .rawsig import CHANNEL_DTYPE, Channel, chunk_table, detect_events_raw_host, to_pa  # noqa: F401
from .seeding import HIT_DTYPE, SeedIndex, SeedParams, seed_hits_host, sketch  # noqa: F401

__all__ = [
    "Engine", "Plan", "DtwResult", "JOB_DTYPE", "ANCHOR_DTYPE", "RAWDTW_FULL",
    "MapOpt", "Chain", "Batch", "CandidateBatch", "ReadCandidates", "align_chain", "evaluate_reads",
    "load_library", "library_path", "LibraryMissing", "RawDTWError",
    "EventOptions", "detect_events", "detect_events_host", "chunks_of",
    "Channel", "CHANNEL_DTYPE", "to_pa", "chunk_table", "detect_events_raw_host",
    "SeedIndex", "SeedParams", "HIT_DTYPE", "sketch", "seed_hits_host",
    "CHAIN_REC_DTYPE", "ROUND_OUT_DTYPE", "round_end_host", "SEED_DTYPE", "round_keep_host", "chain_decline_host",
]

DEFAULT_FOLD_MODE = 4  # rawdtw_set_option("fold_mode"): the library's default chain-fold kernel
