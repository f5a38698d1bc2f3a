"""BGZF in Python (include/bsw_bgzf.h): a block walker that checks every block of a stream with Python's zlib as
the decoder, and a reference writer on zlib's encoder, so the walker tests itself.  No GPU, no library."""

import struct
import zlib
from collections import namedtuple

MAX_BLOCK = 0xff00
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")      # the 16 bytes in front of BSIZE
STORED, FIXED, DYNAMIC = 0, 1, 2

Block = namedtuple("Block", "off size data btype bfinal")


def write(data, block_bytes=MAX_BLOCK, level=1, eof=False):
    """the reference writer: data cut at block_bytes, each chunk one gzip member deflated by zlib; level 0 (and a
    chunk that zlib makes larger than a block may be): the stored form, written here (zlib's own level 0 ends on an
    empty second deflate block)"""
    assert 1 <= block_bytes <= MAX_BLOCK
    out = bytearray()
    for at in range(0, len(data), block_bytes):
        chunk = data[at:at + block_bytes]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = c.compress(chunk) + c.flush()
        if level == 0 or len(body) + 26 > 65536:
            body = b"\x01" + struct.pack("<HH", len(chunk), len(chunk) ^ 0xffff) + chunk
        out += HEAD + struct.pack("<H", len(body) + 25) + body + struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return bytes(out) + (EOF if eof else b"")


def walk(stream, forms=None, eof=None):
    """every block of the stream, checked: the 18 header bytes; BSIZE + 1 the distance to the next block; the payload
    inflates with nothing left over; CRC32 and ISIZE.  forms = (n_stored, n_fixed, n_dynamic): every data block is one
    final deflate block, and the type bits of their first bytes count up to these.  eof True / False: the stream ends
    / does not end with the EOF marker, and no other block is empty.  Raises ValueError."""
    blocks, at = [], 0
    while at < len(stream):
        if len(stream) - at < 26:
            raise ValueError(f"block at {at}: {len(stream) - at} bytes left, a block has at least 26")
        if stream[at:at + 16] != HEAD:
            raise ValueError(f"block at {at}: header {stream[at:at + 16].hex()}")
        size = struct.unpack_from("<H", stream, at + 16)[0] + 1
        if size < 26 or at + size > len(stream):
            raise ValueError(f"block at {at}: BSIZE + 1 = {size} with {len(stream) - at} bytes left")
        if at + size < len(stream) and stream[at + size:at + size + 4] != HEAD[:4]:
            raise ValueError(f"block at {at}: BSIZE + 1 = {size} does not lead to a block")
        payload = stream[at + 18:at + size - 8]
        d = zlib.decompressobj(-15)
        try:
            data = d.decompress(payload)
        except zlib.error as e:
            raise ValueError(f"block at {at}: {e}")
        if not d.eof or d.unused_data or d.unconsumed_tail:
            raise ValueError(f"block at {at}: eof {d.eof}, {len(d.unused_data)} unused bytes")
        crc, isize = struct.unpack_from("<II", stream, at + size - 8)
        if crc != zlib.crc32(data):
            raise ValueError(f"block at {at}: CRC32 {crc:08x}, the data's is {zlib.crc32(data):08x}")
        if isize != len(data) or isize > MAX_BLOCK:
            raise ValueError(f"block at {at}: ISIZE {isize} for {len(data)} bytes")
        blocks.append(Block(at, size, data, (payload[0] >> 1) & 3, payload[0] & 1))
        at += size
    has_eof = bool(blocks) and stream[blocks[-1].off:] == EOF
    body = blocks[:-1] if has_eof else blocks
    if eof is not None:
        if eof != has_eof:
            raise ValueError(f"EOF marker {'missing' if eof else 'present'}")
        if any(not b.data for b in body):
            raise ValueError("an empty block in front of the end")
    if forms is not None:
        if any(not b.bfinal for b in body):
            raise ValueError("a block of more than one deflate block")
        got = tuple(sum(1 for b in body if b.btype == t) for t in (STORED, FIXED, DYNAMIC))
        if got != tuple(forms):
            raise ValueError(f"block types (stored, fixed, dynamic) {got}, the stats say {tuple(forms)}")
    return blocks


def data_blocks(blocks):
    """the blocks but the EOF marker"""
    return blocks[:-1] if blocks and not blocks[-1].data and blocks[-1].size == len(EOF) else blocks


def voff_lands(stream, blocks, voff, base_coffset):
    """(index of the block a virtual offset names, its offset in that block's data); ValueError when it names none"""
    coff, uoff = (int(voff) >> 16) - base_coffset, int(voff) & 0xffff
    for k, b in enumerate(blocks):
        if b.off == coff:
            if uoff > len(b.data):
                raise ValueError(f"offset {uoff} in a block of {len(b.data)} bytes")
            return k, uoff
    raise ValueError(f"no block starts at {coff}")
