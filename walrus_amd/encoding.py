"""Host-side mirror of the walrus-core Red Stuff encoding API over the MI355X engine.

Names, argument meaning and error behaviour follow crates/walrus-core/src/encoding:
  ReedSolomonEncodingConfig  config.rs:416-708 (EncodingFactory methods)
  ReedSolomonEncoder/Decoder basic_encoding.rs:71-430
  SliverData / SliverPair    slivers.rs:48-510
  Symbols / DecodingSymbol   symbols.rs:42-346
  BlobId / metadata          lib.rs:116-189, metadata.rs:337-653
Every computation runs through the C ABI (include/walrus_rs2.h) in libwalrus_rs2.so.
"""

from __future__ import annotations

import base64
import ctypes
import threading
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import AXIS_PRIMARY, AXIS_SECONDARY

PRIMARY = "primary"
SECONDARY = "secondary"
_AXIS = {PRIMARY: AXIS_PRIMARY, SECONDARY: AXIS_SECONDARY}
_ORTHOGONAL = {PRIMARY: SECONDARY, SECONDARY: PRIMARY}
_CHECK = {"skip": _lib.CHECK_SKIP, "default": _lib.CHECK_DEFAULT, "strict": _lib.CHECK_STRICT}
DIGEST_LEN = 32
ENCODING_TYPE_RS2 = 1


# --------------------------------------------------------------------------------------------
# errors (encoding/errors.rs)
# --------------------------------------------------------------------------------------------
class DataTooLargeError(Exception):
    pass


class EncodeError(Exception):
    pass


class InvalidDataSize(EncodeError):
    pass


class IncorrectDataLength(EncodeError):
    def __init__(self, expected: int):
        super().__init__(f"the data length is incorrect (expected: {expected})")
        self.expected = expected


class IncompatibleParameters(EncodeError):
    pass


class DecodeError(Exception):
    pass


class DecoderError(DecodeError):
    """DecodeError::DecoderError(NotEnoughShards ...)"""


class DecodingUnsuccessful(DecodeError):
    pass


class VerificationError(DecodeError):
    pass


class DecodeDataTooLarge(DecodeError):
    pass


class DecodeIncompatibleParameters(DecodeError):
    pass


class DeviceError(RuntimeError):
    pass


def _raise(rc: int, decode: bool = False, expected: int = 0):
    msg = _lib.last_error()
    if rc == _lib.RS2_E_DATA_TOO_LARGE:
        raise (DecodeDataTooLarge(msg) if decode else DataTooLargeError(msg))
    if rc == _lib.RS2_E_EMPTY_DATA:
        raise InvalidDataSize("empty data")
    if rc == _lib.RS2_E_INCORRECT_DATA_LENGTH:
        raise IncorrectDataLength(expected)
    if rc == _lib.RS2_E_INCOMPATIBLE_PARAMETERS:
        raise (DecodeIncompatibleParameters(msg) if decode else IncompatibleParameters(msg))
    if rc == _lib.RS2_E_NOT_ENOUGH_SHARDS:
        raise DecoderError(msg)
    if rc == _lib.RS2_E_DECODING_UNSUCCESSFUL:
        raise DecodingUnsuccessful(msg)
    if rc == _lib.RS2_E_VERIFICATION:
        raise VerificationError(msg)
    if rc == _lib.RS2_E_INVALID_ARGUMENT:
        raise ValueError(msg)
    raise DeviceError(f"rs2 error {rc}: {msg}")


def _ok(rc: int, decode: bool = False, expected: int = 0):
    if rc != _lib.RS2_OK:
        _raise(rc, decode, expected)


RS2_STREAM_LEGACY = 1  # include/walrus_rs2.h: the HIP null stream (torch's default stream)


def _stream(stream: Optional[int]):
    """Stream argument of the plan / verifier ABI: None -> NULL, the engine object's own
    stream; a HIP stream handle (torch.cuda.Stream.cuda_stream) -> that stream.  Handle 0 is
    torch's default (legacy null) stream and is passed as RS2_STREAM_LEGACY, because NULL means
    'own stream' at this ABI: work the caller queued on the default stream (a fill, a copy)
    stays ordered before the engine's kernels."""
    if stream is None:
        return None
    return stream if stream else RS2_STREAM_LEGACY


# --------------------------------------------------------------------------------------------
# parameters (config.rs:717-826, utils.rs:10-25, bft.rs:12-25)
# --------------------------------------------------------------------------------------------
def max_n_faulty(n_shards: int) -> int:
    return (n_shards - 1) // 3


def source_symbols_for_n_shards(n_shards: int) -> Tuple[int, int]:
    p, s = ctypes.c_uint16(), ctypes.c_uint16()
    _ok(_lib.lib().rs2_source_symbols_for_n_shards(n_shards, ctypes.byref(p), ctypes.byref(s)))
    return p.value, s.value


def compute_symbol_size(data_length: int, n_symbols: int, required_alignment: int = 2) -> int:
    data_length = max(data_length, 1)
    size = -(-data_length // n_symbols)
    size = -(-size // required_alignment) * required_alignment
    if size > 0xFFFF:
        raise DataTooLargeError("symbol size too large")
    return size


# --------------------------------------------------------------------------------------------
# containers
# --------------------------------------------------------------------------------------------
class Symbols:
    """Flat symbol container (symbols.rs:42-293)."""

    def __init__(self, data: bytes, symbol_size: int):
        if symbol_size <= 0 or len(data) % symbol_size:
            raise ValueError("data must hold whole symbols")
        self.data = bytes(data)
        self.symbol_size = symbol_size

    def __len__(self):
        return len(self.data) // self.symbol_size

    def __getitem__(self, i: int) -> bytes:
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        s = self.symbol_size
        return self.data[i * s:(i + 1) * s]

    def to_symbols(self) -> List[bytes]:
        return [self[i] for i in range(len(self))]

    def __eq__(self, other):
        return (isinstance(other, Symbols) and self.data == other.data
                and self.symbol_size == other.symbol_size)


@dataclass
class DecodingSymbol:
    """symbols.rs:301-346: a symbol with the index of the sliver/shard it comes from."""
    index: int
    data: bytes


@dataclass
class SliverData:
    """slivers.rs:48-56.  `axis` is PRIMARY or SECONDARY."""
    symbols: Symbols
    index: int
    axis: str = PRIMARY

    def __len__(self):
        return len(self.symbols.data)

    @property
    def symbol_size(self) -> int:
        return self.symbols.symbol_size

    def pair_index(self, n_shards: int) -> int:
        return self.index if self.axis == PRIMARY else n_shards - 1 - self.index

    def recovery_symbols(self, config: "ReedSolomonEncodingConfig") -> Symbols:
        """slivers.rs:169-178: expand on the orthogonal axis to n_shards symbols."""
        return config.encode_all_symbols(_ORTHOGONAL[self.axis], self.symbols.data)

    def get_merkle_root(self, config: "ReedSolomonEncodingConfig") -> bytes:
        """slivers.rs:387-392."""
        out = (ctypes.c_uint8 * 32)()
        data = np.frombuffer(self.symbols.data, dtype=np.uint8)
        _ok(_lib.lib().rs2_sliver_merkle_root(
            config.n_shards, self.symbol_size, _AXIS[self.axis], data.ctypes.data,
            len(data), ctypes.cast(out, ctypes.c_void_p)))
        return bytes(out)

    def decoding_symbol_for_sliver(self, target_pair_index: int,
                                   config: "ReedSolomonEncodingConfig") -> DecodingSymbol:
        """slivers.rs:220-240: the symbol this sliver contributes to another sliver."""
        n = config.n_shards
        orth = _ORTHOGONAL[self.axis]
        target = target_pair_index if orth == PRIMARY else n - 1 - target_pair_index
        return DecodingSymbol(self.index, config.encode_symbol(orth, self.symbols.data, target))

    # ---- wire format ------------------------------------------------------------------------
    # BCS of SliverData<T> (slivers.rs:47-56, symbols.rs:40-49): Symbols { data: Vec<u8> as
    # serde Bytes (ULEB128 length + bytes), symbol_size: NonZeroU16 (u16 LE) }, index:
    # SliverIndex (u16 LE); the PhantomData axis marker serialises to nothing -- the axis is
    # implied by the endpoint that carries it (walrus-storage-node-client/src/client.rs:1035-1047).
    def to_bcs(self) -> bytes:
        n = len(self.symbols.data)
        out = bytearray()
        while True:
            b = n & 0x7F
            n >>= 7
            out.append(b | (0x80 if n else 0))
            if not n:
                break
        out += self.symbols.data
        out += int(self.symbols.symbol_size).to_bytes(2, "little")
        out += int(self.index).to_bytes(2, "little")
        return bytes(out)

    @classmethod
    def from_bcs(cls, raw: bytes, axis: str = PRIMARY) -> "SliverData":
        """Inverse of to_bcs; rejects trailing bytes, over-long / non-canonical ULEB128 lengths,
        a zero symbol size and data that is not whole symbols (as bcs + Symbols::new do)."""
        raw = bytes(raw)
        n, shift, pos = 0, 0, 0
        while True:
            if pos >= len(raw) or shift > 28:
                raise ValueError("bad ULEB128 length")
            b = raw[pos]
            pos += 1
            n |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                if b == 0 and shift > 7:
                    raise ValueError("non-canonical ULEB128 length")
                break
        if n > 0xFFFFFFFF or len(raw) != pos + n + 4:
            raise ValueError("length mismatch")
        data = raw[pos:pos + n]
        symbol_size = int.from_bytes(raw[pos + n:pos + n + 2], "little")
        index = int.from_bytes(raw[pos + n + 2:pos + n + 4], "little")
        if symbol_size == 0:
            raise ValueError("symbol_size must be non-zero")
        return cls(Symbols(data, symbol_size), index, axis)

    def check_hash(self, config: "ReedSolomonEncodingConfig", metadata: "BlobMetadata") -> bool:
        pair = metadata.hashes[self.pair_index(config.n_shards)]
        want = pair[0] if self.axis == PRIMARY else pair[1]
        return self.get_merkle_root(config) == want

    def verify(self, config: "ReedSolomonEncodingConfig", metadata: "BlobMetadata") -> None:
        """slivers.rs:100-121 (raises ValueError on a size mismatch, VerificationError on a
        Merkle-root mismatch)."""
        if self.index >= len(metadata.hashes):
            raise ValueError("IndexTooLarge")
        s = config.symbol_size_for_blob(metadata.unencoded_length)
        k = config.n_secondary_source_symbols if self.axis == PRIMARY else \
            config.n_primary_source_symbols
        if len(self) != k * s:
            raise ValueError("SliverSizeMismatch")
        if self.symbol_size != s:
            raise ValueError("SymbolSizeMismatch")
        if not self.check_hash(config, metadata):
            raise VerificationError("MerkleRootMismatch")

    @staticmethod
    def recover_sliver_from_decoding_symbols(
            symbols: Sequence[DecodingSymbol], target_index: int, symbol_size: int,
            config: "ReedSolomonEncodingConfig", axis: str = PRIMARY) -> "SliverData":
        """slivers.rs:246-289 (recover_sliver_without_verification)."""
        k = config.n_symbols_for_recovery(axis)
        symbols = list(symbols)
        if len(symbols) < k:
            raise DecodingUnsuccessful("not enough recovery symbols")
        data = config.decode_from_decoding_symbols(axis, symbol_size, symbols)
        return SliverData(Symbols(data, symbol_size), target_index, axis)


@dataclass
class SliverPair:
    """slivers.rs:429-510: primary i and secondary n-1-i."""
    primary: SliverData
    secondary: SliverData

    @property
    def index(self) -> int:
        return self.primary.index


class BlobId(bytes):
    """lib.rs:116-189; str() is base64url without padding."""

    def __str__(self):
        return base64.urlsafe_b64encode(bytes(self)).decode().rstrip("=")

    @classmethod
    def from_str(cls, s: str) -> "BlobId":
        return cls(base64.urlsafe_b64decode(s + "=" * (-len(s) % 4)))


@dataclass
class BlobMetadata:
    """metadata.rs:537-653 (V1): per-pair (primary_hash, secondary_hash)."""
    hashes: List[Tuple[bytes, bytes]]
    unencoded_length: int
    encoding_type: int = ENCODING_TYPE_RS2

    def hashes_bytes(self) -> bytes:
        return b"".join(p + s for p, s in self.hashes)

    def compute_blob_id(self) -> BlobId:
        out = (ctypes.c_uint8 * 32)()
        hb = np.frombuffer(self.hashes_bytes(), dtype=np.uint8)
        _ok(_lib.lib().rs2_blob_id_from_hashes(hb.ctypes.data, len(self.hashes),
                                               self.unencoded_length,
                                               ctypes.cast(out, ctypes.c_void_p)))
        return BlobId(bytes(out))


@dataclass
class VerifiedBlobMetadataWithId:
    blob_id: BlobId
    metadata: BlobMetadata

    def verify(self) -> bool:
        return self.metadata.compute_blob_id() == self.blob_id


# --------------------------------------------------------------------------------------------
# 1D codec (basic_encoding.rs)
# --------------------------------------------------------------------------------------------
class ReedSolomonEncoder:
    """basic_encoding.rs:71-342."""

    def __init__(self, symbol_size: int, n_source_symbols: int, n_shards: int):
        if n_shards < n_source_symbols:
            raise IncompatibleParameters("n_shards must be at least n_source_symbols")
        if symbol_size % 2:
            raise IncompatibleParameters(
                "symbol_size must be a multiple of the required alignment")
        self.symbol_size = symbol_size
        self.n_source_symbols = n_source_symbols
        self.n_shards = n_shards

    def _check(self, data: bytes):
        expected = self.n_source_symbols * self.symbol_size
        if len(data) != expected:
            raise IncorrectDataLength(expected)

    def encode_all(self, data: bytes) -> Symbols:
        self._check(data)
        k, n, s = self.n_source_symbols, self.n_shards, self.symbol_size
        out = np.zeros(n * s, dtype=np.uint8)
        src = np.frombuffer(bytes(data), dtype=np.uint8)
        _ok(_lib.lib().rs2_encode_1d(k, n, s, 1, src.ctypes.data, out.ctypes.data))
        return Symbols(out.tobytes(), s)

    def encode_all_repair_symbols(self, data: bytes) -> Symbols:
        allsym = self.encode_all(data)
        return Symbols(allsym.data[self.n_source_symbols * self.symbol_size:], self.symbol_size)

    def get_symbol(self, data: bytes, index: int) -> bytes:
        self._check(data)
        assert index < self.n_shards
        return self.encode_all(data)[index]


class ReedSolomonDecoder:
    """basic_encoding.rs:347-430.  Accumulates symbols across calls until decoding succeeds,
    then resets (basic_encoding.rs:535-566)."""

    def __init__(self, n_source_symbols: int, n_shards: int, symbol_size: int):
        if n_shards <= n_source_symbols or symbol_size % 2:
            raise DecodeIncompatibleParameters("unsupported shard count")
        self.n_source_symbols = n_source_symbols
        self.n_shards = n_shards
        self.symbol_size = symbol_size
        self._pending: "OrderedDict[int, bytes]" = OrderedDict()

    def decode(self, symbols: Iterable[DecodingSymbol]) -> bytes:
        for sym in symbols:
            if len(sym.data) != self.symbol_size:
                continue  # dropped with a warning in the reference
            if sym.index < self.n_shards and sym.index not in self._pending:
                self._pending[sym.index] = bytes(sym.data)
        k, n, s = self.n_source_symbols, self.n_shards, self.symbol_size
        if len(self._pending) < k:
            raise DecoderError("NotEnoughShards")
        idx = (ctypes.c_uint16 * len(self._pending))(*self._pending.keys())
        keep = [np.frombuffer(v, dtype=np.uint8) for v in self._pending.values()]
        ptrs = (ctypes.c_void_p * len(keep))(*[a.ctypes.data for a in keep])
        out = np.zeros(k * s, dtype=np.uint8)
        _ok(_lib.lib().rs2_decode_1d(k, n, s, len(keep), idx, ptrs, out.ctypes.data),
            decode=True)
        self._pending.clear()
        return out.tobytes()


# --------------------------------------------------------------------------------------------
# 2D Red Stuff (config.rs, blob_encoding.rs)
# --------------------------------------------------------------------------------------------
class _Plan:
    def __init__(self, n_shards: int, blob_len: int):
        # a plan serves one call at a time (include/walrus_rs2.h threading rule); threads that
        # share a ReedSolomonEncodingConfig share its plans, so each call holds this lock
        self.lock = threading.Lock()
        self.handle = ctypes.c_void_p()
        rc = _lib.lib().rs2_plan_create(n_shards, blob_len, ctypes.byref(self.handle))
        _ok(rc)
        self.info = _lib.PlanInfo()
        _ok(_lib.lib().rs2_plan_info_get(self.handle, ctypes.byref(self.info)))
        self.blob_len = blob_len

    def bind(self, blob_len: int) -> None:
        """Point the plan at `blob_len` (same symbol size; rs2_plan_rebind).  Call with the
        lock held: the binding is per call."""
        if blob_len != self.blob_len:
            _ok(_lib.lib().rs2_plan_rebind(self.handle, blob_len))
            self.blob_len = blob_len

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and h.value and _lib._LIB is not None:
            _lib.lib().rs2_plan_destroy(h)
            self.handle = ctypes.c_void_p()


class ReedSolomonEncodingConfig:
    """ReedSolomonEncodingConfig / EncodingFactory (config.rs:416-708)."""

    # plans are keyed by symbol size and rebound per call (rs2_plan_rebind): a stream of blobs
    # of many lengths reuses a few plans, whose device buffers come from the bounded arena
    PLAN_CACHE = 4

    def __init__(self, n_shards: int):
        self.n_shards = int(n_shards)
        self.n_primary_source_symbols, self.n_secondary_source_symbols = \
            source_symbols_for_n_shards(self.n_shards)
        self._plans: "OrderedDict[int, _Plan]" = OrderedDict()
        self._plans_lock = threading.Lock()

    # -- parameters ---------------------------------------------------------------------------
    @property
    def source_symbols_primary(self):
        return self.n_primary_source_symbols

    @property
    def source_symbols_secondary(self):
        return self.n_secondary_source_symbols

    def n_source_symbols(self, axis: str) -> int:
        return self.n_primary_source_symbols if axis == PRIMARY else \
            self.n_secondary_source_symbols

    def n_symbols_for_recovery(self, axis: str) -> int:
        """config.rs: symbols to recover a sliver of `axis` = source symbols of the other."""
        return self.n_source_symbols(_ORTHOGONAL[axis])

    def source_symbols_per_blob(self) -> int:
        return self.n_primary_source_symbols * self.n_secondary_source_symbols

    def symbol_size_for_blob(self, blob_size: int) -> int:
        return compute_symbol_size(blob_size, self.source_symbols_per_blob())

    def max_blob_size(self) -> int:
        return self.source_symbols_per_blob() * 0xFFFE

    def encoded_blob_length(self, unencoded_length: int) -> Optional[int]:
        out = ctypes.c_uint64()
        rc = _lib.lib().rs2_encoded_blob_length(self.n_shards, unencoded_length,
                                                ctypes.byref(out))
        return out.value if rc == _lib.RS2_OK else None

    def _plan(self, blob_len: int) -> _Plan:
        """The cached plan of blob_len's symbol size; callers bind() it under its lock."""
        if blob_len > self.max_blob_size():
            return _Plan(self.n_shards, blob_len)  # raises DataTooLargeError like the ABI
        key = self.symbol_size_for_blob(blob_len)
        with self._plans_lock:
            p = self._plans.get(key)
            if p is None:
                p = _Plan(self.n_shards, blob_len)
                self._plans[key] = p
                while len(self._plans) > self.PLAN_CACHE:
                    self._plans.popitem(last=False)  # freed once no call holds it
            else:
                self._plans.move_to_end(key)
            return p

    # -- encode -------------------------------------------------------------------------------
    def encode_with_metadata(self, blob: bytes) -> Tuple[List[SliverPair], VerifiedBlobMetadataWithId]:
        blob = bytes(blob)
        plan = self._plan(len(blob))
        info = plan.info
        n = self.n_shards
        prim = np.zeros((n, info.primary_sliver_len), dtype=np.uint8)
        sec = np.zeros((n, info.secondary_sliver_len), dtype=np.uint8)
        pp = (ctypes.c_void_p * n)(*[prim[i].ctypes.data for i in range(n)])
        sp = (ctypes.c_void_p * n)(*[sec[i].ctypes.data for i in range(n)])
        hashes = np.zeros(n * 64, dtype=np.uint8)
        bid = np.zeros(32, dtype=np.uint8)
        src = np.frombuffer(blob, dtype=np.uint8)
        with plan.lock:
            plan.bind(len(blob))
            _ok(_lib.lib().rs2_encode_with_metadata(
                plan.handle, src.ctypes.data if len(blob) else None, pp, sp, hashes.ctypes.data,
                bid.ctypes.data))
        s = info.symbol_size
        pairs = [SliverPair(SliverData(Symbols(prim[i].tobytes(), s), i, PRIMARY),
                            SliverData(Symbols(sec[n - 1 - i].tobytes(), s), n - 1 - i, SECONDARY))
                 for i in range(n)]
        return pairs, self._metadata(hashes, bid, len(blob))

    def encode_batch_with_metadata(
            self, blobs: Sequence[bytes]) -> List[Tuple[List[SliverPair], VerifiedBlobMetadataWithId]]:
        """encode_with_metadata of many blobs (the upload relay's / client's per-blob loop,
        node_client.rs:3156-3221), one batched device call per group of blobs that share a
        symbol size (rs2_encode_batch_with_metadata).  Same results, in input order."""
        blobs = [bytes(b) for b in blobs]
        n = self.n_shards
        groups: Dict[int, List[int]] = {}
        for i, b in enumerate(blobs):
            groups.setdefault(self.symbol_size_for_blob(len(b)), []).append(i)
        out: List = [None] * len(blobs)
        for s, members in groups.items():
            for c0 in range(0, len(members), 65535):
                chunk = members[c0:c0 + 65535]
                plan = self._plan(max(len(blobs[i]) for i in chunk))
                info = plan.info
                B = len(chunk)
                prim = np.zeros((B, n, info.primary_sliver_len), dtype=np.uint8)
                sec = np.zeros((B, n, info.secondary_sliver_len), dtype=np.uint8)
                hashes = np.zeros(B * n * 64, dtype=np.uint8)
                bids = np.zeros(B * 32, dtype=np.uint8)
                srcs = [np.frombuffer(blobs[i], dtype=np.uint8) for i in chunk]
                bp = (ctypes.c_void_p * B)(*[a.ctypes.data if len(a) else None for a in srcs])
                lens = (ctypes.c_uint64 * B)(*[len(a) for a in srcs])
                pp = (ctypes.c_void_p * (B * n))(*[prim[b, i].ctypes.data for b in range(B)
                                                   for i in range(n)])
                sp = (ctypes.c_void_p * (B * n))(*[sec[b, i].ctypes.data for b in range(B)
                                                   for i in range(n)])
                with plan.lock:
                    plan.bind(max(len(blobs[i]) for i in chunk))
                    _ok(_lib.lib().rs2_encode_batch_with_metadata(
                        plan.handle, B, bp, lens, pp, sp, hashes.ctypes.data, bids.ctypes.data))
                for b, i in enumerate(chunk):
                    pairs = [SliverPair(SliverData(Symbols(prim[b, k].tobytes(), s), k, PRIMARY),
                                        SliverData(Symbols(sec[b, n - 1 - k].tobytes(), s),
                                                   n - 1 - k, SECONDARY))
                             for k in range(n)]
                    out[i] = (pairs, self._metadata(hashes[b * n * 64:(b + 1) * n * 64],
                                                    bids[b * 32:(b + 1) * 32], len(blobs[i])))
        return out

    def encode_blobs_with_metadata(
            self, blobs: Sequence[bytes]) -> List[Tuple[List[SliverPair], VerifiedBlobMetadataWithId]]:
        """encode_with_metadata of many blobs of any lengths (the upload relay's queue): the blobs
        whose symbol size is at least 4 go through ONE call whatever their sizes
        (rs2_encode_blobs_with_metadata), those of symbol size 2 -- every blob of at most
        2 K_p K_s bytes -- through the per-size batch call, which is faster for a uniform batch.
        Same results as encode_batch_with_metadata, in input order."""
        blobs = [bytes(b) for b in blobs]
        n = self.n_shards
        kp, ks = self.n_primary_source_symbols, self.n_secondary_source_symbols
        sizes = [self.symbol_size_for_blob(len(b)) for b in blobs]
        out: List = [None] * len(blobs)
        small = [i for i, s in enumerate(sizes) if s < 4]
        if small:
            for i, r in zip(small, self.encode_batch_with_metadata([blobs[i] for i in small])):
                out[i] = r
        mixed = [i for i, s in enumerate(sizes) if s >= 4]
        for c0 in range(0, len(mixed), 65535):
            chunk = mixed[c0:c0 + 65535]
            B = len(chunk)
            prim = [np.zeros((n, ks * sizes[i]), dtype=np.uint8) for i in chunk]
            sec = [np.zeros((n, kp * sizes[i]), dtype=np.uint8) for i in chunk]
            hashes = np.zeros(B * n * 64, dtype=np.uint8)
            bids = np.zeros(B * 32, dtype=np.uint8)
            srcs = [np.frombuffer(blobs[i], dtype=np.uint8) for i in chunk]
            bp = (ctypes.c_void_p * B)(*[a.ctypes.data for a in srcs])
            lens = (ctypes.c_uint64 * B)(*[len(a) for a in srcs])
            pp = (ctypes.c_void_p * (B * n))(*[prim[b][k].ctypes.data for b in range(B)
                                               for k in range(n)])
            sp = (ctypes.c_void_p * (B * n))(*[sec[b][k].ctypes.data for b in range(B)
                                               for k in range(n)])
            _ok(_lib.lib().rs2_encode_blobs_with_metadata(
                n, B, bp, lens, pp, sp, hashes.ctypes.data, bids.ctypes.data, None))
            for b, i in enumerate(chunk):
                s = sizes[i]
                pairs = [SliverPair(SliverData(Symbols(prim[b][k].tobytes(), s), k, PRIMARY),
                                    SliverData(Symbols(sec[b][n - 1 - k].tobytes(), s),
                                               n - 1 - k, SECONDARY))
                         for k in range(n)]
                out[i] = (pairs, self._metadata(hashes[b * n * 64:(b + 1) * n * 64],
                                                bids[b * 32:(b + 1) * 32], len(blobs[i])))
        return out

    def _metadata(self, hashes: np.ndarray, bid: np.ndarray, blob_len: int):
        hb = hashes.tobytes()
        meta = BlobMetadata([(hb[64 * i:64 * i + 32], hb[64 * i + 32:64 * i + 64])
                             for i in range(self.n_shards)], blob_len)
        return VerifiedBlobMetadataWithId(BlobId(bid.tobytes()), meta)

    def compute_metadata(self, blob: bytes) -> VerifiedBlobMetadataWithId:
        blob = bytes(blob)
        plan = self._plan(len(blob))
        hashes = np.zeros(self.n_shards * 64, dtype=np.uint8)
        bid = np.zeros(32, dtype=np.uint8)
        src = np.frombuffer(blob, dtype=np.uint8)
        with plan.lock:
            plan.bind(len(blob))
            _ok(_lib.lib().rs2_compute_metadata(plan.handle,
                                                src.ctypes.data if len(blob) else None,
                                                hashes.ctypes.data, bid.ctypes.data))
        return self._metadata(hashes, bid, len(blob))

    def compute_blob_id(self, blob: bytes) -> BlobId:
        return self.compute_metadata(blob).blob_id

    # -- decode -------------------------------------------------------------------------------
    def _decode_args(self, slivers: Iterable[SliverData]):
        slivers = list(slivers)
        axes = {s.axis for s in slivers}
        if len(axes) > 1:
            raise ValueError("slivers of both axes")
        axis = axes.pop() if axes else PRIMARY
        keep = [np.frombuffer(s.symbols.data, dtype=np.uint8) for s in slivers]
        m = max(len(slivers), 1)
        idx = (ctypes.c_uint16 * m)(*[s.index for s in slivers])
        ptrs = (ctypes.c_void_p * m)(*[a.ctypes.data for a in keep])
        lens = (ctypes.c_uint64 * m)(*[len(a) for a in keep])
        # symbol sizes travel too: a sliver of the right length but another symbol size is
        # dropped like a wrong-length one (blob_encoding.rs:921-933)
        syms = (ctypes.c_uint16 * m)(*[min(s.symbol_size, 0xFFFF) for s in slivers])
        return axis, slivers, keep, idx, ptrs, lens, syms

    def _decode_plan(self, blob_size: int) -> _Plan:
        try:
            return self._plan(blob_size)
        except DataTooLargeError as e:
            raise DecodeDataTooLarge(str(e))

    def decode(self, blob_size: int, slivers: Iterable[SliverData]) -> bytes:
        """EncodingFactory::decode (config.rs:605-611) / BlobDecoder::decode."""
        axis, slivers, keep, idx, ptrs, lens, syms = self._decode_args(slivers)
        plan = self._decode_plan(blob_size)
        out = np.empty(max(blob_size, 1), dtype=np.uint8)
        with plan.lock:
            plan.bind(blob_size)
            _ok(_lib.lib().rs2_decode_blob(plan.handle, _AXIS[axis], len(slivers), idx, ptrs,
                                           lens, syms, out.ctypes.data), decode=True)
        return out[:blob_size].tobytes()

    def decode_batch(self, blobs: Sequence[Tuple[int, Iterable[SliverData]]]) -> List[bytes]:
        """decode of many blobs, [(blob_size, slivers), ...], one batched device call per group
        of blobs that share a symbol size and an axis (rs2_decode_batch).  Same results as
        decode per blob, in input order; the first failing blob raises its DecodeError."""
        args = [(int(size),) + self._decode_args(slivers) for size, slivers in blobs]
        groups: Dict[Tuple[int, str], List[int]] = {}
        for i, a in enumerate(args):
            if a[0] > self.max_blob_size():
                self._decode_plan(a[0])  # raises DecodeDataTooLarge
            groups.setdefault((self.symbol_size_for_blob(a[0]), a[1]), []).append(i)
        out: List = [None] * len(args)
        for (_, axis), members in groups.items():
            for c0 in range(0, len(members), 65535):
                chunk = members[c0:c0 + 65535]
                B = len(chunk)
                top = max(args[i][0] for i in chunk)
                plan = self._decode_plan(top)
                lens = (ctypes.c_uint64 * B)(*[args[i][0] for i in chunk])
                counts = (ctypes.c_uint32 * B)(*[len(args[i][2]) for i in chunk])
                keep = [a for i in chunk for a in args[i][3]]
                m = max(len(keep), 1)
                idx = (ctypes.c_uint16 * m)(*[s.index for i in chunk for s in args[i][2]])
                ptrs = (ctypes.c_void_p * m)(*[a.ctypes.data for a in keep])
                slens = (ctypes.c_uint64 * m)(*[len(a) for a in keep])
                syms = (ctypes.c_uint16 * m)(*[min(s.symbol_size, 0xFFFF)
                                               for i in chunk for s in args[i][2]])
                outs = [np.empty(max(args[i][0], 1), dtype=np.uint8) for i in chunk]
                op = (ctypes.c_void_p * B)(*[o.ctypes.data for o in outs])
                with plan.lock:
                    plan.bind(top)
                    _ok(_lib.lib().rs2_decode_batch(plan.handle, _AXIS[axis], B, lens, counts, idx,
                                                    ptrs, slens, syms, op, None), decode=True)
                for k, i in enumerate(chunk):
                    out[i] = outs[k][:args[i][0]].tobytes()
        return out

    def decode_and_verify(self, metadata: VerifiedBlobMetadataWithId,
                          slivers: Iterable[SliverData], consistency_check: str = "default") -> bytes:
        """config.rs:613-658 (Default: only the systematic primary slivers that were not among
        the input are re-checked, config.rs:621-640 / blob_encoding.rs:579-612)."""
        axis, slivers, keep, idx, ptrs, lens, syms = self._decode_args(slivers)
        blob_size = metadata.metadata.unencoded_length
        plan = self._decode_plan(blob_size)
        out = np.empty(max(blob_size, 1), dtype=np.uint8)
        check = {"skip": _lib.CHECK_SKIP, "default": _lib.CHECK_DEFAULT,
                 "strict": _lib.CHECK_STRICT}[consistency_check.lower()]
        hb = np.frombuffer(metadata.metadata.hashes_bytes(), dtype=np.uint8)
        bid = np.frombuffer(bytes(metadata.blob_id), dtype=np.uint8)
        with plan.lock:
            plan.bind(blob_size)
            _ok(_lib.lib().rs2_decode_and_verify(plan.handle, _AXIS[axis], len(slivers), idx,
                                                 ptrs, lens, syms, hb.ctypes.data,
                                                 bid.ctypes.data, check, out.ctypes.data),
                decode=True)
        return out[:blob_size].tobytes()

    def decode_and_verify_batch(self, items: Sequence[Tuple[VerifiedBlobMetadataWithId,
                                                            Iterable[SliverData]]],
                                consistency_check: str = "default") -> List[Optional[bytes]]:
        """decode_and_verify of many blobs, [(metadata, slivers), ...], one batched device call
        per group of blobs that share a symbol size and an axis (rs2_decode_and_verify_batch).
        Returns the blob per item, in input order, or None where the check rejected it; a blob
        the decode itself refuses raises its DecodeError, as in decode_batch."""
        check = _CHECK[consistency_check.lower()]
        metas = [m for m, _ in items]
        args = [(int(m.metadata.unencoded_length),) + self._decode_args(slivers)
                for m, slivers in items]
        groups: Dict[Tuple[int, str], List[int]] = {}
        for i, a in enumerate(args):
            if a[0] > self.max_blob_size():
                self._decode_plan(a[0])  # raises DecodeDataTooLarge
            groups.setdefault((self.symbol_size_for_blob(a[0]), a[1]), []).append(i)
        out: List = [None] * len(args)
        for (_, axis), members in groups.items():
            for c0 in range(0, len(members), 65535):
                chunk = members[c0:c0 + 65535]
                B = len(chunk)
                top = max(args[i][0] for i in chunk)
                plan = self._decode_plan(top)
                lens = (ctypes.c_uint64 * B)(*[args[i][0] for i in chunk])
                counts = (ctypes.c_uint32 * B)(*[len(args[i][2]) for i in chunk])
                keep = [a for i in chunk for a in args[i][3]]
                m = max(len(keep), 1)
                idx = (ctypes.c_uint16 * m)(*[s.index for i in chunk for s in args[i][2]])
                ptrs = (ctypes.c_void_p * m)(*[a.ctypes.data for a in keep])
                slens = (ctypes.c_uint64 * m)(*[len(a) for a in keep])
                syms = (ctypes.c_uint16 * m)(*[min(s.symbol_size, 0xFFFF)
                                               for i in chunk for s in args[i][2]])
                hb = np.frombuffer(b"".join(metas[i].metadata.hashes_bytes() for i in chunk),
                                   dtype=np.uint8)
                ids = np.frombuffer(b"".join(bytes(metas[i].blob_id) for i in chunk),
                                    dtype=np.uint8)
                outs = [np.empty(max(args[i][0], 1), dtype=np.uint8) for i in chunk]
                op = (ctypes.c_void_p * B)(*[o.ctypes.data for o in outs])
                verdict = (ctypes.c_int32 * B)()
                with plan.lock:
                    plan.bind(top)
                    _ok(_lib.lib().rs2_decode_and_verify_batch(
                        plan.handle, _AXIS[axis], B, lens, counts, idx, ptrs, slens, syms,
                        hb.ctypes.data, ids.ctypes.data, check, op, verdict, None), decode=True)
                for k, i in enumerate(chunk):
                    if verdict[k] == _lib.RS2_BLOB_MATCH:
                        out[i] = outs[k][:args[i][0]].tobytes()
        return out

    # -- 1D helpers (config.rs:660-707) ----------------------------------------------------------
    def _encoder(self, axis: str, data_len: int) -> ReedSolomonEncoder:
        k = self.n_source_symbols(axis)
        if data_len == 0:
            raise InvalidDataSize("empty data")
        s = compute_symbol_size(data_len, k)
        if data_len != k * s:
            raise IncorrectDataLength(k * s)
        return ReedSolomonEncoder(s, k, self.n_shards)

    def encode_all_symbols(self, axis: str, data: bytes) -> Symbols:
        return self._encoder(axis, len(data)).encode_all(data)

    def encode_all_repair_symbols(self, axis: str, data: bytes) -> Symbols:
        return self._encoder(axis, len(data)).encode_all_repair_symbols(data)

    def encode_symbol(self, axis: str, data: bytes, index: int) -> bytes:
        enc = self._encoder(axis, len(data))
        if index < enc.n_source_symbols:
            s = enc.symbol_size
            return bytes(data[index * s:(index + 1) * s])
        return enc.get_symbol(data, index)

    def decode_from_decoding_symbols(self, axis: str, symbol_size: int,
                                     symbols: Iterable[DecodingSymbol]) -> bytes:
        """Recover a sliver of `axis` from symbols of the orthogonal slivers
        (config.rs:695-707: decoder of the orthogonal axis' code)."""
        k = self.n_source_symbols(_ORTHOGONAL[axis])
        dec = ReedSolomonDecoder(k, self.n_shards, symbol_size)
        return dec.decode(symbols)


def sliver_merkle_roots(config: "ReedSolomonEncodingConfig",
                        slivers: Sequence[SliverData]) -> List[bytes]:
    """SliverData::get_merkle_root (slivers.rs:387-392) for many slivers of one axis and symbol
    size in one device call (rs2_sliver_merkle_roots)."""
    slivers = list(slivers)
    if not slivers:
        return []
    axes = {s.axis for s in slivers}
    sizes = {s.symbol_size for s in slivers}
    if len(axes) != 1 or len(sizes) != 1:
        raise ValueError("slivers must share axis and symbol size")
    keep = [np.frombuffer(s.symbols.data, dtype=np.uint8) for s in slivers]
    ptrs = (ctypes.c_void_p * len(keep))(*[a.ctypes.data for a in keep])
    lens = (ctypes.c_uint64 * len(keep))(*[len(a) for a in keep])
    out = np.zeros(32 * len(keep), dtype=np.uint8)
    _ok(_lib.lib().rs2_sliver_merkle_roots(config.n_shards, sizes.pop(), _AXIS[axes.pop()],
                                           len(keep), ptrs, lens, out.ctypes.data),
        expected=len(keep[0]))
    raw = out.tobytes()
    return [raw[32 * i:32 * i + 32] for i in range(len(keep))]


def verify_slivers(config: "ReedSolomonEncodingConfig", metadata: BlobMetadata,
                   slivers: Sequence[SliverData]) -> List[bool]:
    """SliverData::verify (slivers.rs:100-121) over a batch: True where the sliver's Merkle
    root matches its metadata hash.  Size mismatches raise as in `SliverData.verify`."""
    slivers = list(slivers)
    if not slivers:
        return []
    n = config.n_shards
    s = config.symbol_size_for_blob(metadata.unencoded_length)
    for sl in slivers:
        if sl.index >= len(metadata.hashes):
            raise ValueError("IndexTooLarge")
        k = config.n_secondary_source_symbols if sl.axis == PRIMARY else \
            config.n_primary_source_symbols
        if len(sl) != k * s:
            raise ValueError("SliverSizeMismatch")
        if sl.symbol_size != s:
            raise ValueError("SymbolSizeMismatch")
    result = [False] * len(slivers)
    for axis in (PRIMARY, SECONDARY):
        pos = [i for i, sl in enumerate(slivers) if sl.axis == axis]
        roots = sliver_merkle_roots(config, [slivers[i] for i in pos])
        for i, root in zip(pos, roots):
            pair = metadata.hashes[slivers[i].pair_index(n)]
            result[i] = root == (pair[0] if axis == PRIMARY else pair[1])
    return result


def _mixed_call(n_shards: int, slivers: Sequence[SliverData],
                expected: Optional[bytes]) -> Tuple[List[bytes], Optional[List[int]]]:
    """rs2_verify_slivers_mixed over host slivers: (roots, verdicts or None)."""
    m = len(slivers)
    keep = [np.frombuffer(s.symbols.data, dtype=np.uint8) for s in slivers]
    axes = np.array([_AXIS[s.axis] for s in slivers], dtype=np.uint8)
    sizes = np.array([s.symbol_size for s in slivers], dtype=np.uint16)
    ptrs = (ctypes.c_void_p * m)(*[a.ctypes.data for a in keep])
    lens = (ctypes.c_uint64 * m)(*[len(a) for a in keep])
    roots = np.zeros(32 * m, dtype=np.uint8)
    verdict = np.zeros(m, dtype=np.int32) if expected is not None else None
    exp = np.frombuffer(bytes(expected), dtype=np.uint8) if expected is not None else None
    _ok(_lib.lib().rs2_verify_slivers_mixed(
        n_shards, m, axes.ctypes.data, sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), ptrs,
        lens, exp.ctypes.data if exp is not None else None, roots.ctypes.data,
        verdict.ctypes.data if verdict is not None else None, None))
    raw = roots.tobytes()
    return ([raw[32 * i:32 * i + 32] for i in range(m)],
            [int(v) for v in verdict] if verdict is not None else None)


def sliver_merkle_roots_mixed(config: "ReedSolomonEncodingConfig",
                              slivers: Sequence[SliverData]) -> List[bytes]:
    """SliverData::get_merkle_root (slivers.rs:387-392) for slivers that share only n_shards --
    any mix of axes and symbol sizes -- in one device call (rs2_verify_slivers_mixed)."""
    slivers = list(slivers)
    if not slivers:
        return []
    return _mixed_call(config.n_shards, slivers, None)[0]


def verify_slivers_of_blobs(config: "ReedSolomonEncodingConfig",
                            blobs: Sequence[Tuple[BlobMetadata, Sequence[SliverData]]]
                            ) -> List[List[bool]]:
    """SliverData::verify (slivers.rs:100-121; node.rs:2615-2633 on every received sliver) for
    slivers of many blobs in one device call: per blob, True where the sliver's Merkle root
    matches the hash in that blob's metadata.  Raises as `verify_slivers` does."""
    n = config.n_shards
    blobs = [(metadata, list(slivers)) for metadata, slivers in blobs]
    flat: List[SliverData] = []
    expected = bytearray()
    for metadata, slivers in blobs:
        s = config.symbol_size_for_blob(metadata.unencoded_length)
        for sl in slivers:
            if sl.index >= len(metadata.hashes):
                raise ValueError("IndexTooLarge")
            k = config.n_secondary_source_symbols if sl.axis == PRIMARY else \
                config.n_primary_source_symbols
            if len(sl) != k * s:
                raise ValueError("SliverSizeMismatch")
            if sl.symbol_size != s:
                raise ValueError("SymbolSizeMismatch")
            pair = metadata.hashes[sl.pair_index(n)]
            expected += bytes(pair[0] if sl.axis == PRIMARY else pair[1])
            flat.append(sl)
    verdicts = _mixed_call(n, flat, bytes(expected))[1] if flat else []
    out: List[List[bool]] = []
    at = 0
    for _, slivers in blobs:
        cnt = len(slivers)
        out.append([v == _lib.RS2_SLIVER_MATCH for v in verdicts[at:at + cnt]])
        at += cnt
    return out


def verify_mixed_stats() -> Dict[str, int]:
    """rs2_verify_mixed_stats: windows of the mixed sliver verification calls, slivers verified
    inside group launches, slivers that took the per-size path, groups (distinct axis / symbol
    size pairs inside windows) and compute launches of the group path (process-wide)."""
    out = (ctypes.c_uint64 * 5)()
    _ok(_lib.lib().rs2_verify_mixed_stats(out))
    return dict(zip(("windows", "grouped", "single", "groups", "launches"),
                    (int(v) for v in out)))


def symbols_mixed_stats() -> Dict[str, int]:
    """rs2_symbols_mixed_stats: windows of the mixed recovery-symbol calls, slivers expanded,
    trees built, trees served from the caller's cache, requests served and compute launches of
    the group path (process-wide)."""
    out = (ctypes.c_uint64 * 6)()
    _ok(_lib.lib().rs2_symbols_mixed_stats(out))
    return dict(zip(("windows", "expanded", "built", "cached", "requests", "launches"),
                    (int(v) for v in out)))


def set_verify_mixed_budget(nbytes: int = 0) -> None:
    """rs2_set_verify_mixed_budget: scratch a window of a mixed sliver verification may hold
    (0 restores the 256 MiB default)."""
    _ok(_lib.lib().rs2_set_verify_mixed_budget(int(nbytes)))


def encode_mixed_stats() -> Dict[str, int]:
    """rs2_encode_mixed_stats: windows of the mixed blob encode calls, blobs encoded inside group
    launches, blobs that took the per-blob path, distinct symbol sizes inside windows and compute
    launches of the group path (process-wide)."""
    out = (ctypes.c_uint64 * 5)()
    _ok(_lib.lib().rs2_encode_mixed_stats(out))
    return dict(zip(("windows", "grouped", "single", "sizes", "launches"),
                    (int(v) for v in out)))


def set_encode_mixed_budget(nbytes: int = 0) -> None:
    """rs2_set_encode_mixed_budget: scratch a window of a mixed blob encode may hold (0 restores
    the 4 GiB default)."""
    _ok(_lib.lib().rs2_set_encode_mixed_budget(int(nbytes)))


class BlobEncoder:
    """Device-resident blob encode across sizes (rs2_blob_encoder_*): bound to n_shards only; every
    blob of a call has its own length, hence its own symbol size, and its own place in device
    memory."""

    WINDOW_LAUNCHES = _lib.RS2_ENCODE_MIXED_WINDOW_LAUNCHES
    WINDOW_BLOBS = _lib.RS2_ENCODE_MIXED_WINDOW_BLOBS

    def __init__(self, n_shards: int):
        self.handle = ctypes.c_void_p()
        _ok(_lib.lib().rs2_blob_encoder_create(n_shards, ctypes.byref(self.handle)))

    def encode_async(self, blob_lens: Sequence[int], d_blobs: int, blob_offsets: Sequence[int],
                     d_primary: int, primary_offsets: Optional[Sequence[int]], d_secondary: int,
                     secondary_offsets: Optional[Sequence[int]], d_hashes: int, d_blob_ids: int,
                     stream: Optional[int] = None, statuses: bool = False):
        """rs2_blob_encoder_encode_device_async: blob b (blob_lens[b] bytes) lies at d_blobs +
        blob_offsets[b]; its primary / secondary slivers go to d_primary + primary_offsets[b] /
        d_secondary + secondary_offsets[b] (the single-blob layouts), its pair hashes to
        d_hashes + b*64*n and its id to d_blob_ids + b*32.  d_primary and d_secondary 0: metadata
        only.  With `statuses` the per-blob codes are returned and failing blobs skipped;
        without, the status code of the call is returned (the first failure, nothing enqueued)."""
        m = len(blob_lens)

        def u64(v):
            if v is None:
                return None
            a = np.array(list(v) + [0], dtype=np.uint64)
            return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))

        lens, boff = u64(blob_lens), u64(blob_offsets)
        poff, soff = u64(primary_offsets), u64(secondary_offsets)
        st = (ctypes.c_int * max(m, 1))() if statuses else None
        rc = _lib.lib().rs2_blob_encoder_encode_device_async(
            self.handle, m, lens[1], d_blobs or None, boff[1], d_primary or None,
            poff[1] if poff else None, d_secondary or None, soff[1] if soff else None,
            d_hashes or None, d_blob_ids or None, st, _stream(stream))
        if statuses:
            _ok(rc)
            return list(st)[:m]
        return rc

    def stats(self) -> Dict[str, int]:
        return encode_mixed_stats()

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and h.value and _lib._LIB is not None:
            _lib.lib().rs2_blob_encoder_destroy(h)
            self.handle = ctypes.c_void_p()


class SliverChecker:
    """Device-resident sliver verification across blobs (rs2_sliver_checker_*): bound to n_shards
    only; every sliver of a call has its own axis, symbol size and place in device memory."""

    def __init__(self, n_shards: int):
        self.handle = ctypes.c_void_p()
        _ok(_lib.lib().rs2_sliver_checker_create(n_shards, ctypes.byref(self.handle)))

    def verify_async(self, axes: Sequence[str], symbol_sizes: Sequence[int], d_base: int,
                     offsets: Sequence[int], expected_roots: Optional[bytes] = None,
                     d_roots: int = 0, d_verdict: int = 0, stream: Optional[int] = None,
                     statuses: bool = False):
        """rs2_sliver_checker_verify_device_async: sliver i (axes[i], symbol_sizes[i]) lies at
        d_base + offsets[i]; its root goes to d_roots + 32 i and, with expected_roots, its
        RS2_SLIVER_* verdict to d_verdict + 4 i.  With `statuses` the per-sliver codes are
        returned and failing slivers skipped; without, the status code of the call is returned
        (the first failure, nothing enqueued)."""
        m = len(axes)
        ax = np.array([_AXIS.get(a, a) for a in axes] + [0], dtype=np.uint8)
        sz = np.array(list(symbol_sizes) + [0], dtype=np.uint16)
        off = np.array(list(offsets) + [0], dtype=np.uint64)
        exp = None
        if expected_roots is not None:
            exp = np.frombuffer(bytes(expected_roots) or b"\0", dtype=np.uint8)
        st = (ctypes.c_int * max(m, 1))() if statuses else None
        rc = _lib.lib().rs2_sliver_checker_verify_device_async(
            self.handle, m, ax.ctypes.data, sz.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)),
            d_base or None, off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            exp.ctypes.data if exp is not None else None, d_roots or None, d_verdict or None, st,
            _stream(stream))
        if statuses:
            _ok(rc)
            return list(st)[:m]
        return rc

    def recover_async(self, axes: Sequence[str], symbol_sizes: Sequence[int],
                      index_lists: Sequence[Sequence[int]], d_symbols_base: int,
                      symbols_off: Sequence[int], d_slivers_base: int, sliver_off: Sequence[int],
                      expected_roots: Optional[bytes] = None, d_roots: int = 0,
                      d_verdict: int = 0, stream: Optional[int] = None, statuses: bool = False):
        """rs2_sliver_checker_recover_device_async: sliver i (axes[i], symbol_sizes[i]) is
        recovered from the received symbols whose source indices are index_lists[i], their data
        back to back at d_symbols_base + symbols_off[i], and written at d_slivers_base +
        sliver_off[i].  Roots, verdicts, `statuses` and the return value as verify_async."""
        m = len(axes)
        ax = np.array([_AXIS.get(a, a) for a in axes] + [0], dtype=np.uint8)
        sz = np.array(list(symbol_sizes) + [0], dtype=np.uint16)
        counts = np.array([len(x) for x in index_lists] + [0], dtype=np.uint32)
        idx = np.array([i for x in index_lists for i in x] + [0], dtype=np.uint16)
        s_off = np.array(list(symbols_off) + [0], dtype=np.uint64)
        o_off = np.array(list(sliver_off) + [0], dtype=np.uint64)
        exp = None
        if expected_roots is not None:
            exp = np.frombuffer(bytes(expected_roots) or b"\0", dtype=np.uint8)
        st = (ctypes.c_int * max(m, 1))() if statuses else None
        u16, u32, u64 = (ctypes.POINTER(t) for t in (ctypes.c_uint16, ctypes.c_uint32,
                                                     ctypes.c_uint64))
        rc = _lib.lib().rs2_sliver_checker_recover_device_async(
            self.handle, m, ax.ctypes.data, sz.ctypes.data_as(u16), counts.ctypes.data_as(u32),
            idx.ctypes.data_as(u16), d_symbols_base or None, s_off.ctypes.data_as(u64),
            exp.ctypes.data if exp is not None else None, d_slivers_base or None,
            o_off.ctypes.data_as(u64), d_roots or None, d_verdict or None, st, _stream(stream))
        if statuses:
            _ok(rc)
            return list(st)[:m]
        return rc

    def recovery_symbols_async(self, axes: Sequence[str], symbol_sizes: Sequence[int],
                               d_slivers_base: int, sliver_off: Sequence[int],
                               targets_per_sliver: Sequence[Sequence[int]], d_symbols_base: int,
                               symbols_off: Sequence[int], d_proofs: int, d_nodes: int = 0,
                               trees: str = "build", stream: Optional[int] = None,
                               statuses: bool = False):
        """rs2_sliver_checker_recovery_symbols_device_async: source sliver i (axes[i],
        symbol_sizes[i]) lies at d_slivers_base + sliver_off[i] and serves targets_per_sliver[i]
        (orthogonal-axis indices); its symbols go back to back to d_symbols_base +
        symbols_off[i], request j of the concatenated lists gets its Merkle path at d_proofs +
        j*path_len*32, and sliver i's tree is d_nodes + i*n_nodes*32.  trees "build" / "cached"
        as SliverVerifier.recovery_symbols_multi_async; `statuses` and the return value as
        verify_async."""
        m = len(axes)
        ax = np.array([_AXIS.get(a, a) for a in axes] + [0], dtype=np.uint8)
        sz = np.array(list(symbol_sizes) + [0], dtype=np.uint16)
        counts = np.array([len(x) for x in targets_per_sliver] + [0], dtype=np.uint32)
        tg = np.array([t for x in targets_per_sliver for t in x] + [0], dtype=np.uint16)
        i_off = np.array(list(sliver_off) + [0], dtype=np.uint64)
        o_off = np.array(list(symbols_off) + [0], dtype=np.uint64)
        mode = {"build": _lib.RS2_TREES_BUILD, "cached": _lib.RS2_TREES_CACHED}.get(trees, trees)
        st = (ctypes.c_int * max(m, 1))() if statuses else None
        u16, u32, u64 = (ctypes.POINTER(t) for t in (ctypes.c_uint16, ctypes.c_uint32,
                                                     ctypes.c_uint64))
        rc = _lib.lib().rs2_sliver_checker_recovery_symbols_device_async(
            self.handle, m, ax.ctypes.data, sz.ctypes.data_as(u16), d_slivers_base or None,
            i_off.ctypes.data_as(u64), counts.ctypes.data_as(u32), tg.ctypes.data_as(u16), mode,
            d_nodes or None, d_symbols_base or None, o_off.ctypes.data_as(u64), d_proofs or None,
            st, _stream(stream))
        if statuses:
            _ok(rc)
            return list(st)[:m]
        return rc

    def check_recovery_symbols_async(self, symbol_sizes: Sequence[int], counts: Sequence[int],
                                     targets: Sequence[int], d_symbols_base: int,
                                     symbols_off: Sequence[int], d_proofs: int,
                                     d_expected_roots: int, d_ok: int,
                                     stream: Optional[int] = None) -> int:
        """rs2_sliver_checker_check_recovery_symbols_device_async (returns the status code)."""
        m = len(counts)
        return _lib.lib().rs2_sliver_checker_check_recovery_symbols_device_async(
            self.handle, m, (ctypes.c_uint16 * max(m, 1))(*symbol_sizes),
            (ctypes.c_uint32 * max(m, 1))(*counts), (ctypes.c_uint16 * max(m, 1))(*targets),
            d_symbols_base or None, (ctypes.c_uint64 * max(m, 1))(*symbols_off),
            d_proofs or None, d_expected_roots or None, d_ok or None, _stream(stream))

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and h.value and _lib._LIB is not None:
            _lib.lib().rs2_sliver_checker_destroy(h)
            self.handle = ctypes.c_void_p()


class SliverVerifier:
    """Device-resident batched sliver verification (rs2_verifier_*): Merkle roots of `count`
    back-to-back device slivers of one axis into a device buffer."""

    def __init__(self, n_shards: int, symbol_size: int, axis: str = PRIMARY):
        self.handle = ctypes.c_void_p()
        _ok(_lib.lib().rs2_verifier_create(n_shards, symbol_size, _AXIS[axis],
                                           ctypes.byref(self.handle)))

    def roots_async(self, count: int, d_slivers: int, d_roots: int,
                    stream: Optional[int] = None) -> None:
        _ok(_lib.lib().rs2_verifier_roots_device_async(self.handle, count, d_slivers, d_roots,
                                                       _stream(stream)))

    def recovery_symbols_async(self, count: int, d_slivers: int, targets: Sequence[int],
                               d_symbols: int, d_proofs: int, d_nodes: int = 0,
                               stream: Optional[int] = None) -> None:
        """rs2_verifier_recovery_symbols_device_async: request i expands source sliver i and
        returns its symbol targets[i] (orthogonal-axis index) and that leaf's Merkle path; with
        d_nodes, every tree's node array too (recovery_symbol_service.rs:132-235)."""
        tg = (ctypes.c_uint16 * count)(*targets)
        _ok(_lib.lib().rs2_verifier_recovery_symbols_device_async(
            self.handle, count, d_slivers, tg, d_symbols, d_proofs, d_nodes or None,
            _stream(stream)))

    def recovery_symbols_multi_async(self, d_slivers: int,
                                     targets_per_sliver: Sequence[Sequence[int]],
                                     d_symbols: int, d_proofs: int, d_nodes: int = 0,
                                     trees: str = "build", stream: Optional[int] = None) -> int:
        """rs2_verifier_recovery_symbols_multi_device_async (returns the status code): source
        sliver i (back to back in d_slivers) serves targets_per_sliver[i] (orthogonal-axis
        indices); request j of the concatenated lists gets its symbol at d_symbols + j*s and its
        Merkle path at d_proofs + j*path_len*32.  trees "build": every sliver is expanded and
        hashed once and its tree built (into d_nodes when given, which also warms slivers
        without targets); "cached": the trees are read from d_nodes and nothing is hashed."""
        m = len(targets_per_sliver)
        counts = (ctypes.c_uint32 * max(m, 1))(*[len(x) for x in targets_per_sliver])
        flat = [t for x in targets_per_sliver for t in x]
        tg = (ctypes.c_uint16 * max(len(flat), 1))(*flat)
        mode = {"build": _lib.RS2_TREES_BUILD, "cached": _lib.RS2_TREES_CACHED}.get(trees, trees)
        return _lib.lib().rs2_verifier_recovery_symbols_multi_device_async(
            self.handle, m, d_slivers or None, counts, tg, mode, d_nodes or None,
            d_symbols or None, d_proofs or None, _stream(stream))

    def recover_slivers_async(self, index_lists: Sequence[Sequence[int]], d_symbols: int,
                              d_slivers_out: int, expected_roots: Optional[bytes] = None,
                              d_roots: int = 0, d_verdict: int = 0,
                              stream: Optional[int] = None, statuses: bool = False):
        """rs2_verifier_recover_slivers_device_async: sliver i is recovered from the received
        symbols whose source indices are index_lists[i], their data back to back in d_symbols in
        the same order.  With `statuses` the per-sliver codes are returned and failing slivers
        skipped; without, the first failure raises and nothing is enqueued."""
        m = len(index_lists)
        counts = (ctypes.c_uint32 * max(m, 1))(*[len(x) for x in index_lists])
        flat = [i for x in index_lists for i in x]
        idx = (ctypes.c_uint16 * max(len(flat), 1))(*flat)
        exp = None
        if expected_roots is not None:
            exp = (ctypes.c_uint8 * max(len(expected_roots), 1)).from_buffer_copy(
                bytes(expected_roots) or b"\0")
        st = (ctypes.c_int * max(m, 1))() if statuses else None
        rc = _lib.lib().rs2_verifier_recover_slivers_device_async(
            self.handle, m, counts, idx, d_symbols or None, exp, d_slivers_out or None,
            d_roots or None, d_verdict or None, st, _stream(stream))
        if statuses:
            _ok(rc)
            return list(st)[:m]
        return rc

    def check_recovery_symbols_async(self, counts: Sequence[int], targets: Sequence[int],
                                     d_symbols: int, d_proofs: int, d_expected_roots: int,
                                     d_ok: int, stream: Optional[int] = None) -> int:
        """rs2_verifier_check_recovery_symbols_device_async (returns the status code)."""
        m = len(counts)
        return _lib.lib().rs2_verifier_check_recovery_symbols_device_async(
            self.handle, m, (ctypes.c_uint32 * max(m, 1))(*counts),
            (ctypes.c_uint16 * max(m, 1))(*targets), d_symbols or None, d_proofs or None,
            d_expected_roots or None, d_ok or None, _stream(stream))

    def profile(self, enable: bool = True) -> None:
        _ok(_lib.lib().rs2_verifier_profile_enable(self.handle, int(enable)))

    def profile_read(self) -> dict:
        """{stage: (total_ms, launches)} of the recovery calls since the last read
        (synchronises)."""
        m = 64
        names = ctypes.create_string_buffer(32 * m)
        ms = (ctypes.c_double * m)()
        cnt = (ctypes.c_uint32 * m)()
        k = ctypes.c_uint32()
        _ok(_lib.lib().rs2_verifier_profile_read(self.handle, m, names, ms, cnt,
                                                 ctypes.byref(k)))
        raw = names.raw
        return {raw[32 * i:32 * i + 32].split(b"\0")[0].decode(): (ms[i], cnt[i])
                for i in range(k.value)}

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and h.value and _lib._LIB is not None:
            _lib.lib().rs2_verifier_destroy(h)
            self.handle = ctypes.c_void_p()


def device_memory_stats(device: int = 0) -> Dict[str, int]:
    """rs2_device_memory_stats: the device arena's hipMalloc / hipFree counts and bytes."""
    out = (ctypes.c_uint64 * 7)()
    _ok(_lib.lib().rs2_device_memory_stats(device, out))
    keys = ("mallocs", "frees", "live", "reserved", "peak", "syncs", "pinned_allocs")
    return dict(zip(keys, (int(v) for v in out)))


def upload_stats() -> Dict[str, int]:
    """rs2_upload_stats: uploads through the pinned slot ring, codec jobs through the job ring,
    and slot reuses that waited for the slot's previous copy (its completion word)."""
    out = (ctypes.c_uint64 * 3)()
    _ok(_lib.lib().rs2_upload_stats(out))
    return dict(zip(("uploads", "jobs", "waits"), (int(v) for v in out)))


def decode_batch_stats() -> Dict[str, int]:
    """rs2_decode_batch_stats: batched decode launches, blobs decoded inside them, and blobs of
    batch calls that took the per-blob path (process-wide)."""
    out = (ctypes.c_uint64 * 3)()
    _ok(_lib.lib().rs2_decode_batch_stats(out))
    return dict(zip(("launches", "batched", "single"), (int(v) for v in out)))


def verify_batch_stats() -> Dict[str, int]:
    """rs2_verify_batch_stats: check windows of verified decode batches, blobs checked (Default
    or Strict), rows hashed by Default, blobs re-encoded by Strict (process-wide)."""
    out = (ctypes.c_uint64 * 4)()
    _ok(_lib.lib().rs2_verify_batch_stats(out))
    return dict(zip(("windows", "checked", "rows", "encoded"), (int(v) for v in out)))


def set_verify_batch_budget(nbytes: int = 0) -> None:
    """rs2_set_verify_batch_budget: check scratch a window of a verified decode batch may hold
    (0 restores the 256 MiB default)."""
    _ok(_lib.lib().rs2_set_verify_batch_budget(int(nbytes)))


def recover_stats() -> Dict[str, int]:
    """rs2_recover_stats: batched sliver-recovery launches, slivers decoded inside them, and
    slivers of recovery calls that took the per-sliver path (process-wide)."""
    out = (ctypes.c_uint64 * 3)()
    _ok(_lib.lib().rs2_recover_stats(out))
    return dict(zip(("launches", "batched", "single"), (int(v) for v in out)))


def recover_mixed_stats() -> Dict[str, int]:
    """rs2_recover_mixed_stats: windows of the mixed sliver-recovery calls, decode range launches,
    slivers decoded inside them, slivers that took the per-sliver decode path and groups (distinct
    axis / symbol size pairs inside windows) (process-wide)."""
    out = (ctypes.c_uint64 * 5)()
    _ok(_lib.lib().rs2_recover_mixed_stats(out))
    return dict(zip(("windows", "launches", "batched", "single", "groups"),
                    (int(v) for v in out)))


def recovery_symbols_stats() -> Dict[str, int]:
    """rs2_recovery_symbols_stats: windows of the bulk recovery-symbol calls, slivers expanded,
    trees built, trees taken from the caller's cache, requests served (process-wide)."""
    out = (ctypes.c_uint64 * 5)()
    _ok(_lib.lib().rs2_recovery_symbols_stats(out))
    return dict(zip(("windows", "expanded", "built", "cached", "requests"),
                    (int(v) for v in out)))


def set_recovery_symbols_budget(nbytes: int = 0) -> None:
    """rs2_set_recovery_symbols_budget: device scratch a window of a bulk recovery-symbol call
    may hold (0 restores the 256 MiB default)."""
    _ok(_lib.lib().rs2_set_recovery_symbols_budget(int(nbytes)))


def device_memory_trim(device: int = 0) -> int:
    """rs2_device_memory_trim: hand the arena's wholly free segments back; returns the bytes."""
    out = ctypes.c_uint64()
    _ok(_lib.lib().rs2_device_memory_trim(device, ctypes.byref(out)))
    return int(out.value)


# --------------------------------------------------------------------------------------------
# device-resident plan (the measured path): pointers are device addresses (e.g. torch tensors)
# --------------------------------------------------------------------------------------------
class DevicePlan:
    """rs2_encode_device_async / rs2_decode_device_async on caller-owned device buffers."""

    def __init__(self, n_shards: int, blob_len: int):
        self._plan = _Plan(n_shards, blob_len)
        self.info = self._plan.info

    @property
    def handle(self):
        return self._plan.handle

    def encode_async(self, d_blob: int, d_primary: int, d_secondary: int, d_hashes: int,
                     d_blob_id: int, stream: Optional[int] = None) -> None:
        _ok(_lib.lib().rs2_encode_device_async(self.handle, d_blob, d_primary, d_secondary,
                                               d_hashes, d_blob_id, _stream(stream)))

    def compute_metadata_async(self, d_blob: int, d_hashes: int, d_blob_id: int,
                               stream: Optional[int] = None) -> None:
        """rs2_compute_metadata_device_async: BlobEncoder::compute_metadata on a device blob
        (pair hashes + BlobId only; the slivers stay in the plan's scratch)."""
        _ok(_lib.lib().rs2_compute_metadata_device_async(self.handle, d_blob, d_hashes,
                                                         d_blob_id, _stream(stream)))

    def encode_split_async(self, d_blob: int, d_primary: int, d_secondary: int, d_hashes: int,
                           d_blob_id: int, stream: Optional[int], primary_stream: int) -> None:
        """encode_async, with `primary_stream` released as soon as the primary slivers are
        written (the secondary codecs and hashing continue on `stream`)."""
        _ok(_lib.lib().rs2_encode_device_split_async(self.handle, d_blob, d_primary, d_secondary,
                                                     d_hashes, d_blob_id, _stream(stream),
                                                     _stream(primary_stream)))

    def encode_batch_async(self, n_blobs: int, d_blobs: int, blob_stride: int,
                           blob_lens: Optional[Sequence[int]], d_primary: int, primary_stride: int,
                           d_secondary: int, secondary_stride: int, d_hashes: int,
                           d_blob_ids: int, stream: Optional[int] = None) -> None:
        """rs2_encode_batch_device_async: n_blobs blobs of this plan's symbol size, blob b at
        d_blobs + b*blob_stride (blob_lens[b] bytes, None = the plan's blob_len), its slivers at
        d_primary + b*primary_stride / d_secondary + b*secondary_stride, its pair hashes at
        d_hashes + b*64n and BlobId at d_blob_ids + b*32; one launch per stage."""
        lens = (ctypes.c_uint64 * n_blobs)(*blob_lens) if blob_lens is not None else None
        _ok(_lib.lib().rs2_encode_batch_device_async(
            self.handle, n_blobs, d_blobs, blob_stride, lens, d_primary, primary_stride,
            d_secondary, secondary_stride, d_hashes, d_blob_ids, _stream(stream)))

    def decode_async(self, axis: str, indices: Sequence[int], d_base: int,
                     offsets: Sequence[int], d_out: int, stream: Optional[int] = None) -> None:
        n = len(indices)
        idx = (ctypes.c_uint16 * n)(*indices)
        off = (ctypes.c_uint64 * n)(*offsets)
        _ok(_lib.lib().rs2_decode_device_async(self.handle, _AXIS[axis], n, idx, d_base, off,
                                               d_out, _stream(stream)), decode=True)

    def decode_batch_async(self, axis: str, blobs: Sequence[Tuple[Sequence[int], Sequence[int]]],
                           d_base: int, d_out: int, out_stride: int,
                           blob_lens: Optional[Sequence[int]] = None,
                           stream: Optional[int] = None,
                           statuses: bool = False) -> Optional[List[int]]:
        """rs2_decode_batch_device_async: blob b is decoded from the slivers
        blobs[b] = (indices, offsets from d_base) into d_out + b*out_stride (blob_lens[b] bytes,
        None = the plan's blob_len).  statuses=False: the first invalid blob raises and nothing
        is enqueued; True: invalid blobs are skipped and the per-blob codes are returned."""
        B = len(blobs)
        counts = (ctypes.c_uint32 * max(B, 1))(*[len(ix) for ix, _ in blobs])
        # (numpy: index / offset arrays pass through without a per-element conversion)
        idx = np.concatenate([np.asarray(ix, dtype=np.uint16) for ix, _ in blobs] +
                             [np.zeros(1, dtype=np.uint16)])
        off = np.concatenate([np.asarray(of, dtype=np.uint64) for _, of in blobs] +
                             [np.zeros(1, dtype=np.uint64)])
        lens = (ctypes.c_uint64 * max(B, 1))(*blob_lens) if blob_lens is not None else None
        status = (ctypes.c_int * max(B, 1))() if statuses else None
        _ok(_lib.lib().rs2_decode_batch_device_async(
            self.handle, _AXIS[axis], B, lens, counts,
            idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), d_base,
            off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), d_out, out_stride,
            status, _stream(stream)), decode=True)
        return [int(v) for v in status[:B]] if statuses else None

    def decode_and_verify_batch_async(self, axis: str,
                                      blobs: Sequence[Tuple[Sequence[int], Sequence[int]]],
                                      d_base: int, d_out: int, out_stride: int, d_hashes: int,
                                      d_blob_ids: int, check: str, d_verdict: int,
                                      blob_lens: Optional[Sequence[int]] = None,
                                      stream: Optional[int] = None,
                                      statuses: bool = False) -> Optional[List[int]]:
        """rs2_decode_and_verify_batch_device_async: decode_batch_async plus the consistency
        check ("skip" / "default" / "strict") of every blob against its own device-resident
        metadata (blob b's pair hashes at d_hashes + b*64n, its id at d_blob_ids + b*32; 0 for
        the one the check does not read).  d_verdict receives an int32 per blob (RS2_BLOB_*);
        nothing is read back and the stream is not synchronised."""
        B = len(blobs)
        counts = (ctypes.c_uint32 * max(B, 1))(*[len(ix) for ix, _ in blobs])
        idx = np.concatenate([np.asarray(ix, dtype=np.uint16) for ix, _ in blobs] +
                             [np.zeros(1, dtype=np.uint16)])
        off = np.concatenate([np.asarray(of, dtype=np.uint64) for _, of in blobs] +
                             [np.zeros(1, dtype=np.uint64)])
        lens = (ctypes.c_uint64 * max(B, 1))(*blob_lens) if blob_lens is not None else None
        status = (ctypes.c_int * max(B, 1))() if statuses else None
        _ok(_lib.lib().rs2_decode_and_verify_batch_device_async(
            self.handle, _AXIS[axis], B, lens, counts,
            idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), d_base,
            off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), d_hashes or None,
            d_blob_ids or None, _CHECK[check.lower()], d_out, out_stride, d_verdict,
            status, _stream(stream)), decode=True)
        return [int(v) for v in status[:B]] if statuses else None

    def decode_and_verify(self, axis: str, indices: Sequence[int], d_base: int,
                          offsets: Sequence[int], hashes: bytes, blob_id: bytes, check: str,
                          d_out: int, stream: Optional[int] = None) -> None:
        """rs2_decode_and_verify_device: decode into d_out and run the consistency check
        ("skip" / "default" / "strict", config.rs:613-658) on the device; returns once the
        verdict is known (DecodeError kinds as ReedSolomonEncodingConfig.decode_and_verify)."""
        n = len(indices)
        idx = (ctypes.c_uint16 * n)(*indices)
        off = (ctypes.c_uint64 * n)(*offsets)
        mode = {"skip": _lib.CHECK_SKIP, "default": _lib.CHECK_DEFAULT,
                "strict": _lib.CHECK_STRICT}[check.lower()]
        hb = np.frombuffer(bytes(hashes), dtype=np.uint8)
        bid = np.frombuffer(bytes(blob_id), dtype=np.uint8)
        _ok(_lib.lib().rs2_decode_and_verify_device(
            self.handle, _AXIS[axis], n, idx, d_base, off, hb.ctypes.data, bid.ctypes.data, mode,
            d_out, _stream(stream)), decode=True)

    def sync(self, stream: Optional[int] = None) -> None:
        _ok(_lib.lib().rs2_sync(self.handle, _stream(stream)))

    def profile(self, enable: bool = True) -> None:
        _ok(_lib.lib().rs2_profile_enable(self.handle, int(enable)))

    def profile_read(self) -> dict:
        """{stage: (total_ms, launches)} since the last read (synchronises)."""
        m = 64
        names = ctypes.create_string_buffer(32 * m)
        ms = (ctypes.c_double * m)()
        cnt = (ctypes.c_uint32 * m)()
        k = ctypes.c_uint32()
        _ok(_lib.lib().rs2_profile_read(self.handle, m, names, ms, cnt, ctypes.byref(k)))
        raw = names.raw
        return {raw[32 * i:32 * i + 32].split(b"\0")[0].decode(): (ms[i], cnt[i])
                for i in range(k.value)}
