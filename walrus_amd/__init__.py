"""walrus_amd: MI355X-native Red Stuff (RS2) erasure-coding engine for Walrus.

The hot path (2D sliver encode, Blake2b Merkle metadata, blob decode / sliver recovery) runs
as HIP kernels for gfx950 in libwalrus_rs2.so behind the C ABI of include/walrus_rs2.h.
`walrus_amd.encoding` mirrors the crates/walrus-core encoding API on top of it.
"""

from . import _lib
from . import mapping  # noqa: F401  (sliver pair <-> shard rotation)
from . import quilt  # noqa: F401  (QuiltV1 layout, index, encoder/decoder)
from . import recovery  # noqa: F401  (recovery symbols, Merkle proofs, inconsistency proofs)
from .encoding import (  # noqa: F401
    PRIMARY,
    SECONDARY,
    BlobEncoder,
    BlobId,
    BlobMetadata,
    DataTooLargeError,
    DecodeError,
    DecoderError,
    DecodingSymbol,
    DecodingUnsuccessful,
    DevicePlan,
    EncodeError,
    IncompatibleParameters,
    IncorrectDataLength,
    ReedSolomonDecoder,
    ReedSolomonEncoder,
    ReedSolomonEncodingConfig,
    SliverChecker,
    SliverData,
    SliverPair,
    SliverVerifier,
    Symbols,
    VerificationError,
    VerifiedBlobMetadataWithId,
    compute_symbol_size,
    encode_mixed_stats,
    recover_mixed_stats,
    recovery_symbols_stats,
    set_encode_mixed_budget,
    set_recovery_symbols_budget,
    set_verify_batch_budget,
    set_verify_mixed_budget,
    sliver_merkle_roots,
    sliver_merkle_roots_mixed,
    source_symbols_for_n_shards,
    symbols_mixed_stats,
    verify_batch_stats,
    verify_mixed_stats,
    verify_slivers,
    verify_slivers_of_blobs,
)

from .recovery import (  # noqa: F401
    GeneralRecoverySymbol,
    InconsistencyProof,
    MerkleProof,
    RecoverySymbol,
    recover_sliver_or_generate_inconsistency_proof,
    recover_slivers_of_blobs,
    recover_slivers_or_generate_inconsistency_proofs,
    recovery_symbol_for_sliver,
    recovery_symbols_for_requests,
    recovery_symbols_for_targets,
    recovery_symbols_of_blobs,
    try_recover_sliver_from_decoding_symbols,
    verify_recovery_symbols,
    verify_recovery_symbols_of_blobs,
)

build_library = _lib.build_library
device_available = _lib.device_available

__all__ = [n for n in dir() if not n.startswith("_")]
