"""Reader of TensorFlow's tf.train.Saver V2 checkpoints: `model.ckpt-<step>.index` + `model.ckpt-<step>.data-*-of-*`.

The reference restores the `ScoreNet` and `Temporal` scopes from such a checkpoint (`RestoreFromScope`, KFNet/eval.py:66-68,
KFNet/train.py:317-321).  This module reads the format with Python, numpy and the library's `kfn_crc32c`; it needs neither
TensorFlow nor protobuf nor snappy packages.

    python -m kfnet_amd.checkpoint list PREFIX                       # name, dtype, shape of every tensor
    python -m kfnet_amd.checkpoint to-npz PREFIX OUT.npz [--scope S]  # the kfnet_weights*.npz container

The format ("TensorFlow checkpoints"):
  - `.index` is a LevelDB-style sorted table.  Its last 48 bytes are the footer: the metaindex and index block handles
    (varint64 offset, size), zero padding to 40 bytes, the magic 0xdb4775248b80fb57 (fixed64).  Every block is followed by
    a type byte (0 raw, 1 snappy) and the masked CRC-32C of the stored bytes plus that type byte.  A block holds prefix-
    compressed entries (varint32 shared, non-shared, value length; key delta; value), then a uint32 restart array and its
    count.  The index block's values are the handles of the data blocks, whose keys ascend strictly.
  - Key "" holds a BundleHeaderProto (num_shards, endianness, version); every other key a tensor name whose value is a
    BundleEntryProto (dtype, shape, shard_id, offset, size, masked crc32c, slices).
  - The tensor is `size` raw little-endian bytes at `offset` of `PREFIX.data-<shard_id>-of-<num_shards>` (%05d each).
Every block and every tensor read is checksummed; only the tensors asked for are read (a training checkpoint's Adam slots,
about two thirds of its data, are never touched by `load_checkpoint`).  Not supported, and refused with a message: V1
checkpoints (one `model.ckpt-N` file), partitioned variables (`slices`), string tensors.
"""
import argparse
import ctypes
import os
import struct
import sys
import time

import numpy as np

TABLE_MAGIC = 0xdb4775248b80fb57
FOOTER_BYTES = 48
BLOCK_TRAILER_BYTES = 5
BLOCK_RAW, BLOCK_SNAPPY = 0, 1
MASK_DELTA = 0xa282ead8
DEFAULT_SCOPES = ('ScoreNet', 'Temporal')

# DataType enum (tensorflow/core/framework/types.proto) -> (name, numpy dtype of the stored bytes)
DTYPES = {1: ('float32', '<f4'), 2: ('float64', '<f8'), 3: ('int32', '<i4'), 4: ('uint8', 'u1'), 5: ('int16', '<i2'),
          6: ('int8', 'i1'), 9: ('int64', '<i8'), 10: ('bool', '?'), 14: ('bfloat16', '<u2'), 19: ('float16', '<f2')}
DTYPE_NAMES = {7: 'string', 8: 'complex64', 11: 'qint8', 12: 'quint8', 13: 'qint32', 15: 'qint16', 16: 'quint16',
               17: 'uint16', 18: 'complex128', 20: 'resource', 21: 'variant', 22: 'uint32', 23: 'uint64'}
FLOAT_DTYPES = ('float32', 'float64', 'bfloat16', 'float16')


class CheckpointError(ValueError):
    """A checkpoint that is malformed, corrupt or outside what this reader supports."""


# ---- CRC-32C (kfn_crc32c) -----------------------------------------------------------------------------------------------

def crc32c(data, crc=0):
    """CRC-32C of a bytes-like object, extending `crc` (0 starts a checksum), computed by the library's native host code."""
    from . import _lib
    a = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data.reshape(-1).view(np.uint8)
    if a.size and not a.flags.c_contiguous:
        a = np.ascontiguousarray(a)
    c = ctypes.c_uint32(crc)
    _lib.check(_lib.load().kfn_crc32c(a.ctypes.data if a.size else None, a.size, ctypes.byref(c)), 'kfn_crc32c')
    return c.value


def mask(crc):
    """LevelDB / TF: the stored form of a CRC that covers data which may itself contain CRCs."""
    return ((((crc >> 15) | (crc << 17)) & 0xffffffff) + MASK_DELTA) & 0xffffffff


def unmask(masked):
    rot = (masked - MASK_DELTA) & 0xffffffff
    return ((rot >> 17) | (rot << 15)) & 0xffffffff


# ---- varints, snappy ----------------------------------------------------------------------------------------------------

def _varint(buf, pos, bits=64, what='varint'):
    """(value, next position) of the unsigned varint at buf[pos]."""
    result, shift, end = 0, 0, pos + (bits + 6) // 7
    while True:
        if pos >= len(buf):
            raise CheckpointError('truncated %s' % what)
        if pos == end:
            raise CheckpointError('%s longer than %d bits' % (what, bits))
        b = buf[pos]
        pos += 1
        result |= (b & 0x7f) << shift
        if not b & 0x80:
            break
        shift += 7
    if result >> bits:
        raise CheckpointError('%s longer than %d bits' % (what, bits))
    return result, pos


def snappy_decompress(data):
    """Raw snappy format: varint uncompressed length, then literal and copy elements (1-, 2- and 4-byte offsets;
    a copy may overlap its own output).  Malformed streams raise CheckpointError."""
    data = memoryview(data).cast('B') if not isinstance(data, (bytes, bytearray)) else data
    n, pos = _varint(data, 0, 32, 'snappy length')
    out = bytearray()
    end = len(data)
    while pos < end:
        tag = data[pos]
        pos += 1
        kind = tag & 3
        if kind == 0:
            ln = tag >> 2
            if ln >= 60:
                nb = ln - 59
                if pos + nb > end:
                    raise CheckpointError('snappy: truncated literal length')
                ln = int.from_bytes(bytes(data[pos:pos + nb]), 'little')
                pos += nb
            ln += 1
            if pos + ln > end:
                raise CheckpointError('snappy: literal runs past the input')
            if len(out) + ln > n:
                raise CheckpointError('snappy: output longer than the declared %d bytes' % n)
            out += data[pos:pos + ln]
            pos += ln
            continue
        if kind == 1:
            if pos + 1 > end:
                raise CheckpointError('snappy: truncated copy')
            ln = 4 + ((tag >> 2) & 7)
            off = ((tag >> 5) << 8) | data[pos]
            pos += 1
        else:
            nb = 2 if kind == 2 else 4
            if pos + nb > end:
                raise CheckpointError('snappy: truncated copy')
            ln = (tag >> 2) + 1
            off = int.from_bytes(bytes(data[pos:pos + nb]), 'little')
            pos += nb
        if off == 0 or off > len(out):
            raise CheckpointError('snappy: copy offset %d outside the %d bytes written' % (off, len(out)))
        if len(out) + ln > n:
            raise CheckpointError('snappy: output longer than the declared %d bytes' % n)
        start = len(out) - off
        if off >= ln:
            out += out[start:start + ln]
        else:                                   # overlapping: the last `off` bytes repeat
            pat = bytes(out[start:])
            out += (pat * (ln // off + 1))[:ln]
    if len(out) != n:
        raise CheckpointError('snappy: %d bytes decoded, %d declared' % (len(out), n))
    return bytes(out)


# ---- the sorted table (.index) ------------------------------------------------------------------------------------------

def _block_handle(buf, pos, what):
    off, pos = _varint(buf, pos, 64, what)
    size, pos = _varint(buf, pos, 64, what)
    return off, size, pos


def _read_block(data, off, size, path):
    """Contents of the block at (off, size) of the table file `data`, after its CRC check and decompression."""
    if off + size + BLOCK_TRAILER_BYTES > len(data) - FOOTER_BYTES:
        raise CheckpointError('%s: block at %d (+%d bytes) runs past the end of the file (truncated?)' % (path, off, size))
    stored = data[off:off + size + 1]
    kind = stored[size]
    want = unmask(struct.unpack_from('<I', data, off + size + 1)[0])
    got = crc32c(stored)
    if got != want:
        raise CheckpointError('%s: CRC-32C mismatch in the block at offset %d (stored %08x, computed %08x)'
                              % (path, off, want, got))
    if kind == BLOCK_RAW:
        return bytes(stored[:size])
    if kind == BLOCK_SNAPPY:
        try:
            return snappy_decompress(stored[:size])
        except CheckpointError as e:
            raise CheckpointError('%s: block at offset %d: %s' % (path, off, e))
    raise CheckpointError('%s: block at offset %d has compression type %d (only 0 = raw and 1 = snappy are known)'
                          % (path, off, kind))


def _block_entries(block, path):
    """[(key, value)] of one block (prefix-compressed keys, restart array at the end)."""
    if len(block) < 4:
        raise CheckpointError('%s: block of %d bytes has no restart count' % (path, len(block)))
    nrestart = struct.unpack_from('<I', block, len(block) - 4)[0]
    limit = len(block) - 4 - 4 * nrestart
    if limit < 0:
        raise CheckpointError('%s: block restart array (%d entries) larger than the block' % (path, nrestart))
    out, pos, key = [], 0, b''
    while pos < limit:
        shared, pos = _varint(block, pos, 32, 'block entry')
        nonshared, pos = _varint(block, pos, 32, 'block entry')
        vlen, pos = _varint(block, pos, 32, 'block entry')
        if shared > len(key) or pos + nonshared + vlen > limit:
            raise CheckpointError('%s: corrupt block entry' % path)
        key = key[:shared] + block[pos:pos + nonshared]
        pos += nonshared
        out.append((key, block[pos:pos + vlen]))
        pos += vlen
    return out


def read_table(path):
    """[(key bytes, value bytes)] of a LevelDB-style table file, in order; keys must ascend strictly."""
    with open(path, 'rb') as f:
        data = f.read()
    if len(data) < FOOTER_BYTES:
        raise CheckpointError('%s: %d bytes, shorter than a table footer (truncated?)' % (path, len(data)))
    foot = data[-FOOTER_BYTES:]
    magic = struct.unpack_from('<Q', foot, 40)[0]
    if magic != TABLE_MAGIC:
        raise CheckpointError('%s: bad table magic %016x (not a TF V2 checkpoint index, or truncated)' % (path, magic))
    _, _, p = _block_handle(foot, 0, 'footer')      # metaindex: unused (no filter blocks in checkpoints)
    ioff, isize, _ = _block_handle(foot, p, 'footer')
    entries = []
    for _, handle in _block_entries(_read_block(data, ioff, isize, path), path):
        off, size, _ = _block_handle(handle, 0, 'index entry')
        for key, value in _block_entries(_read_block(data, off, size, path), path):
            if entries and key <= entries[-1][0]:
                raise CheckpointError('%s: keys out of order (%r after %r)' % (path, key, entries[-1][0]))
            entries.append((key, value))
    return entries


# ---- protobuf wire format -----------------------------------------------------------------------------------------------

def _fields(buf, what):
    """(field number, wire type, value) of a serialized message: an int for varint / fixed fields, bytes for
    length-delimited ones.  Unknown fields are the caller's to skip."""
    pos = 0
    while pos < len(buf):
        key, pos = _varint(buf, pos, 64, what)
        num, wt = key >> 3, key & 7
        if wt == 0:
            v, pos = _varint(buf, pos, 64, what)
        elif wt == 1:
            if pos + 8 > len(buf):
                raise CheckpointError('truncated %s' % what)
            v = struct.unpack_from('<Q', buf, pos)[0]
            pos += 8
        elif wt == 5:
            if pos + 4 > len(buf):
                raise CheckpointError('truncated %s' % what)
            v = struct.unpack_from('<I', buf, pos)[0]
            pos += 4
        elif wt == 2:
            ln, pos = _varint(buf, pos, 64, what)
            if pos + ln > len(buf):
                raise CheckpointError('truncated %s' % what)
            v = bytes(buf[pos:pos + ln])
            pos += ln
        else:
            raise CheckpointError('%s: unsupported wire type %d (field %d)' % (what, wt, num))
        yield num, wt, v


def _int64(v):
    return v - (1 << 64) if v >> 63 else v


def parse_header(buf):
    """BundleHeaderProto -> dict(num_shards, endianness, producer, min_consumer)."""
    h = dict(num_shards=0, endianness=0, producer=0, min_consumer=0)
    for num, wt, v in _fields(buf, 'BundleHeaderProto'):
        if num == 1 and wt == 0:
            h['num_shards'] = _int64(v)
        elif num == 2 and wt == 0:
            h['endianness'] = v
        elif num == 3 and wt == 2:
            for n2, w2, v2 in _fields(v, 'VersionDef'):
                if n2 == 1 and w2 == 0:
                    h['producer'] = _int64(v2)
                elif n2 == 2 and w2 == 0:
                    h['min_consumer'] = _int64(v2)
    return h


def parse_entry(buf):
    """BundleEntryProto -> dict(dtype, shape, shard_id, offset, size, crc32c (masked), slices)."""
    e = dict(dtype=0, shape=(), shard_id=0, offset=0, size=0, crc32c=0, slices=0)
    dims = []
    for num, wt, v in _fields(buf, 'BundleEntryProto'):
        if num == 1 and wt == 0:
            e['dtype'] = v
        elif num == 2 and wt == 2:
            for n2, w2, v2 in _fields(v, 'TensorShapeProto'):
                if n2 == 2 and w2 == 2:
                    size = 0
                    for n3, w3, v3 in _fields(v2, 'TensorShapeProto.Dim'):
                        if n3 == 1 and w3 == 0:
                            size = _int64(v3)
                    dims.append(size)
                elif n2 == 3 and w2 == 0 and v2:
                    dims = None                 # unknown_rank
                    break
        elif num in (3, 4, 5) and wt == 0:
            e[{3: 'shard_id', 4: 'offset', 5: 'size'}[num]] = _int64(v)
        elif num == 6 and wt == 5:
            e['crc32c'] = v
        elif num == 7 and wt == 2:
            e['slices'] += 1
    e['shape'] = None if dims is None else tuple(dims)
    return e


def dtype_name(code):
    if code in DTYPES:
        return DTYPES[code][0]
    return DTYPE_NAMES.get(code, 'dtype(%d)' % code)


# ---- the bundle ---------------------------------------------------------------------------------------------------------

class Checkpoint(object):
    """A V2 checkpoint named by its prefix (`.../model.ckpt-2500`).  Opening reads and checks the `.index` table; tensor
    bytes are read by `read(name)` alone.  `timings` accumulates the seconds spent reading data files ('read') and
    checksumming them ('crc'), and the bytes read ('bytes')."""

    def __init__(self, prefix):
        self.prefix = prefix
        self.index_path = prefix + '.index'
        if not os.path.exists(self.index_path):
            if os.path.isfile(prefix):
                raise CheckpointError('%s looks like a V1 checkpoint (one file, no .index): only V2 checkpoints '
                                      '(<prefix>.index + <prefix>.data-*) are supported' % prefix)
            raise CheckpointError('%s: no such checkpoint (%s is missing)' % (prefix, self.index_path))
        table = read_table(self.index_path)
        if not table or table[0][0] != b'':
            raise CheckpointError('%s: no bundle header (key "")' % self.index_path)
        self.header = parse_header(table[0][1])
        if self.header['endianness'] != 0:
            raise CheckpointError('%s: big-endian checkpoint (endianness %d) is not supported'
                                  % (self.index_path, self.header['endianness']))
        if self.header['num_shards'] < 1:
            raise CheckpointError('%s: num_shards = %d' % (self.index_path, self.header['num_shards']))
        if self.header['min_consumer'] > 1:
            raise CheckpointError('%s: needs a reader of bundle version >= %d (this one reads version 1)'
                                  % (self.index_path, self.header['min_consumer']))
        self._entries = {}
        for key, value in table[1:]:
            try:
                name = key.decode('utf-8')
            except UnicodeDecodeError:
                raise CheckpointError('%s: tensor name %r is not UTF-8' % (self.index_path, key))
            try:
                self._entries[name] = parse_entry(value)
            except CheckpointError as err:
                raise CheckpointError('%s: entry %s: %s' % (self.index_path, name, err))
        self.timings = dict(read=0.0, crc=0.0, bytes=0)

    def names(self):
        return sorted(self._entries)

    def __contains__(self, name):
        return name in self._entries

    def _entry(self, name):
        try:
            return self._entries[name]
        except KeyError:
            raise KeyError('%s: no tensor %r' % (self.prefix, name))

    def dtype(self, name):
        """The TF dtype's name ('float32', 'int64', 'bfloat16', 'string', ...)."""
        return dtype_name(self._entry(name)['dtype'])

    def shape(self, name):
        return self._entry(name)['shape']

    def data_path(self, shard_id):
        return '%s.data-%05d-of-%05d' % (self.prefix, shard_id, self.header['num_shards'])

    def read(self, name):
        """The tensor as a numpy array of its shape (bfloat16 is widened to float32, exactly), after checking its size
        and its CRC-32C against the entry."""
        e = self._entry(name)
        if e['slices']:
            raise CheckpointError('%s: %s is a partitioned variable (%d slices); not supported'
                                  % (self.prefix, name, e['slices']))
        if e['dtype'] not in DTYPES:
            raise CheckpointError('%s: %s has dtype %s, which has no fixed item size; not supported'
                                  % (self.prefix, name, self.dtype(name)))
        shape = e['shape']
        if shape is None or any(d < 0 for d in shape):
            raise CheckpointError('%s: %s has an unknown shape %s' % (self.prefix, name, shape))
        npdt = np.dtype(DTYPES[e['dtype']][1])
        want = npdt.itemsize * int(np.prod(shape, dtype=np.int64))
        if e['size'] != want:
            raise CheckpointError('%s: %s holds %d bytes, but %s %s needs %d'
                                  % (self.prefix, name, e['size'], self.dtype(name), list(shape), want))
        if not 0 <= e['shard_id'] < self.header['num_shards']:
            raise CheckpointError('%s: %s is in shard %d of %d' % (self.prefix, name, e['shard_id'],
                                                                   self.header['num_shards']))
        path = self.data_path(e['shard_id'])
        if not os.path.exists(path):
            raise CheckpointError('%s: data file %s is missing' % (self.prefix, path))
        t0 = time.perf_counter()
        buf = bytearray(want)
        with open(path, 'rb') as f:
            f.seek(e['offset'])
            got = f.readinto(buf) if want else 0
        t1 = time.perf_counter()
        if got != want:
            raise CheckpointError('%s: %s: %s ends after %d of its %d bytes (truncated?)'
                                  % (self.prefix, name, path, got, want))
        crc = crc32c(buf)
        self.timings['read'] += t1 - t0
        self.timings['crc'] += time.perf_counter() - t1
        self.timings['bytes'] += want
        if crc != unmask(e['crc32c']):
            raise CheckpointError('%s: CRC-32C mismatch in variable %s (data file %s, offset %d: stored %08x, '
                                  'computed %08x)' % (self.prefix, name, path, e['offset'], unmask(e['crc32c']), crc))
        a = np.frombuffer(buf, npdt).reshape(shape)
        if e['dtype'] == 14:                    # bfloat16: the high half of a float32
            a = (a.astype(np.uint32) << 16).view(np.float32)
        return a


def model_variables(scopes=DEFAULT_SCOPES):
    """{tf_variable_name: shape} of the prediction path's variables under `scopes` (kfnet_amd.weights.variable_specs)."""
    from .weights import variable_specs
    out = {}
    for name, kind, shape in variable_specs():
        if name.split('/')[0] in scopes:
            out[name + '/kernel'] = tuple(shape)
            out[name + '/bias'] = (shape[2] if kind == 'deconv' else shape[-1],)
    return out


def restore(prefix, scopes=DEFAULT_SCOPES):
    """(weights, checkpoint): see load_checkpoint; the Checkpoint carries the names and the timings."""
    ck = Checkpoint(prefix)
    W = {}
    for name, shape in model_variables(scopes).items():
        if name not in ck:
            continue
        if ck.dtype(name) not in FLOAT_DTYPES:
            raise ValueError('%s: model variable %s has dtype %s, not a float type' % (prefix, name, ck.dtype(name)))
        if ck.shape(name) != shape:
            raise ValueError('%s: variable %s has shape %s, the model needs %s'
                             % (prefix, name, list(ck.shape(name) or ()), list(shape)))
        W[name] = ck.read(name).astype(np.float32, copy=False)
    return W, ck


def load_checkpoint(prefix, scopes=DEFAULT_SCOPES):
    """{tf_variable_name: float32 array} of the model variables under `scopes` that the checkpoint holds -- what
    `weights.load_npz` returns for a `.npz` container.  Everything else (Adam slots, beta*_power, global_step, ...) is
    ignored and never read.  A shape that differs from the model's, or a non-float model variable, is a ValueError."""
    return restore(prefix, scopes)[0]


# ---- command line -------------------------------------------------------------------------------------------------------

def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m kfnet_amd.checkpoint', description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd')
    p = sub.add_parser('list', help='name, dtype and shape of every tensor')
    p.add_argument('prefix')
    p = sub.add_parser('to-npz', help='write the model variables as a kfnet_weights .npz container')
    p.add_argument('prefix')
    p.add_argument('out')
    p.add_argument('--scope', action='append', help='variable scope to convert (repeatable; default ScoreNet, Temporal)')
    a = ap.parse_args(argv)
    if a.cmd is None:
        ap.print_usage(sys.stderr)
        return 2
    try:
        if a.cmd == 'list':
            ck = Checkpoint(a.prefix)
            for name in ck.names():
                print('%s (%s) %s' % (name, ck.dtype(name), list(ck.shape(name)) if ck.shape(name) is not None else '?'))
            return 0
        from .weights import save_npz
        W, ck = restore(a.prefix, tuple(a.scope) if a.scope else DEFAULT_SCOPES)
        save_npz(a.out, W)
        print('%s: %d variables written, %d ignored' % (a.out, len(W), len(ck.names()) - len(W)))
        return 0
    except (CheckpointError, ValueError, OSError) as e:
        print('error: %s' % e, file=sys.stderr)
        return 1


if __name__ == '__main__':
    sys.exit(main())
