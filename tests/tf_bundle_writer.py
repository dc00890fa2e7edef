"""Test-only writer of TensorFlow V2 checkpoints (tf.train.Saver's `<prefix>.index` + `<prefix>.data-*-of-*`), written
from the format's description and independent of kfnet_amd.checkpoint (which it must not import): the header and entry
messages are encoded by google.protobuf from descriptors built here, the `.index` table by a LevelDB-style table builder
with a choice of block size, restart interval and compression (raw or snappy), and tensors may be spread over shards.

CRC-32C comes from the library's kfn_crc32c, which tests/test_checkpoint_host.py checks against a bitwise CRC.
"""
import ctypes
import struct

import numpy as np

TABLE_MAGIC = 0xdb4775248b80fb57
MASK_DELTA = 0xa282ead8

# numpy dtype -> TF DataType enum (tensorflow/core/framework/types.proto)
TF_DTYPES = {np.dtype('float32'): 1, np.dtype('float64'): 2, np.dtype('int32'): 3, np.dtype('uint8'): 4,
             np.dtype('int16'): 5, np.dtype('int8'): 6, np.dtype('int64'): 9, np.dtype('bool'): 10,
             np.dtype('float16'): 19}
DT_STRING, DT_BFLOAT16 = 7, 14

_messages = None


def messages():
    """{name: message class} of the tensorflow protos a bundle holds, from descriptors built here (proto3)."""
    global _messages
    if _messages is not None:
        return _messages
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    F = descriptor_pb2.FieldDescriptorProto
    fdp = descriptor_pb2.FileDescriptorProto(name='kfnet_test_tensor_bundle.proto', package='tensorflow', syntax='proto3')

    def msg(parent, name, fields):
        m = parent.add(name=name)
        for fname, num, typ, label, type_name in fields:
            f = m.field.add(name=fname, number=num, type=typ, label=label)
            if type_name:
                f.type_name = type_name
        return m

    opt, rep = F.LABEL_OPTIONAL, F.LABEL_REPEATED
    msg(fdp.message_type, 'VersionDef', [('producer', 1, F.TYPE_INT32, opt, None),
                                         ('min_consumer', 2, F.TYPE_INT32, opt, None),
                                         ('bad_consumers', 3, F.TYPE_INT32, rep, None)])
    shape = msg(fdp.message_type, 'TensorShapeProto', [('dim', 2, F.TYPE_MESSAGE, rep, '.tensorflow.TensorShapeProto.Dim'),
                                                       ('unknown_rank', 3, F.TYPE_BOOL, opt, None)])
    msg(shape.nested_type, 'Dim', [('size', 1, F.TYPE_INT64, opt, None), ('name', 2, F.TYPE_STRING, opt, None)])
    sl = msg(fdp.message_type, 'TensorSliceProto', [('extent', 1, F.TYPE_MESSAGE, rep, '.tensorflow.TensorSliceProto.Extent')])
    msg(sl.nested_type, 'Extent', [('start', 1, F.TYPE_INT64, opt, None), ('length', 2, F.TYPE_INT64, opt, None)])
    hdr = msg(fdp.message_type, 'BundleHeaderProto', [
        ('num_shards', 1, F.TYPE_INT32, opt, None),
        ('endianness', 2, F.TYPE_ENUM, opt, '.tensorflow.BundleHeaderProto.Endianness'),
        ('version', 3, F.TYPE_MESSAGE, opt, '.tensorflow.VersionDef')])
    en = hdr.enum_type.add(name='Endianness')
    en.value.add(name='LITTLE', number=0)
    en.value.add(name='BIG', number=1)
    msg(fdp.message_type, 'BundleEntryProto', [
        ('dtype', 1, F.TYPE_INT32, opt, None),          # the DataType enum: the same varint on the wire
        ('shape', 2, F.TYPE_MESSAGE, opt, '.tensorflow.TensorShapeProto'),
        ('shard_id', 3, F.TYPE_INT32, opt, None),
        ('offset', 4, F.TYPE_INT64, opt, None),
        ('size', 5, F.TYPE_INT64, opt, None),
        ('crc32c', 6, F.TYPE_FIXED32, opt, None),
        ('slices', 7, F.TYPE_MESSAGE, rep, '.tensorflow.TensorSliceProto')])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fdp)
    _messages = {n: message_factory.GetMessageClass(pool.FindMessageTypeByName('tensorflow.' + n))
                 for n in ('VersionDef', 'TensorShapeProto', 'TensorSliceProto', 'BundleHeaderProto', 'BundleEntryProto')}
    return _messages


# ---- CRC ----------------------------------------------------------------------------------------------------------------

def crc32c(data):
    from kfnet_amd import _lib
    a = np.frombuffer(bytes(data), np.uint8)
    c = ctypes.c_uint32(0)
    assert _lib.load().kfn_crc32c(a.ctypes.data if a.size else None, a.size, ctypes.byref(c)) == 0
    return c.value


def mask(c):
    return ((((c >> 15) | (c << 17)) & 0xffffffff) + MASK_DELTA) & 0xffffffff


# ---- snappy (raw format) ------------------------------------------------------------------------------------------------

def varint(v):
    out = bytearray()
    while True:
        b = v & 0x7f
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def snappy_literal(b):
    n = len(b) - 1
    if n < 60:
        return bytes([n << 2]) + bytes(b)
    nb = (n.bit_length() + 7) // 8
    return bytes([(59 + nb) << 2]) + n.to_bytes(nb, 'little') + bytes(b)


def snappy_copy(offset, length, width=None):
    """One copy element; `width` (1, 2, 4) forces the offset size, else the shortest that fits."""
    if width is None:
        width = 1 if (4 <= length <= 11 and offset < 2048) else (2 if offset < 65536 else 4)
    if width == 1:
        assert 4 <= length <= 11 and offset < 2048
        return bytes([1 | ((length - 4) << 2) | ((offset >> 8) << 5), offset & 0xff])
    assert 1 <= length <= 64
    return bytes([(2 if width == 2 else 3) | ((length - 1) << 2)]) + offset.to_bytes(width, 'little')


def snappy_compress(data):
    """A greedy LZ77 over a 4-byte hash: literals, copies with 1-, 2- and 4-byte offsets (the last only past 64 KiB),
    overlapping copies for runs."""
    data = bytes(data)
    out = bytearray(varint(len(data)))
    table, i, lit = {}, 0, 0
    n = len(data)
    while i + 4 <= n:
        key = data[i:i + 4]
        cand = table.get(key)
        table[key] = i
        if cand is None:
            i += 1
            continue
        ln = 4
        while i + ln < n and ln < 64 and data[cand + ln] == data[i + ln]:
            ln += 1
        if lit < i:
            out += snappy_literal(data[lit:i])
        out += snappy_copy(i - cand, ln)
        i += ln
        lit = i
    if lit < n:
        out += snappy_literal(data[lit:])
    return bytes(out)


# ---- the table (.index) -------------------------------------------------------------------------------------------------

def build_block(entries, restart_interval):
    out, restarts, prev = bytearray(), [], b''
    for k, (key, value) in enumerate(entries):
        if k % restart_interval == 0:
            restarts.append(len(out))
            shared = 0
        else:
            shared = 0
            while shared < min(len(prev), len(key)) and prev[shared] == key[shared]:
                shared += 1
        out += varint(shared) + varint(len(key) - shared) + varint(len(value)) + key[shared:] + value
        prev = key
    if not restarts:
        restarts = [0]
    for r in restarts:
        out += struct.pack('<I', r)
    out += struct.pack('<I', len(restarts))
    return bytes(out)


def write_table(path, entries, block_size=4096, restart_interval=16, compression='raw', check_order=True):
    """A LevelDB-style table of (key, value) byte pairs (given in order).  compression: 'raw' or 'snappy' (every block,
    even where it does not shrink), or an int: the type byte written as is (with the raw bytes)."""
    if check_order:
        assert all(a[0] < b[0] for a, b in zip(entries, entries[1:]))
    f = bytearray()

    def put_block(contents):
        if compression == 'snappy':
            stored, kind = snappy_compress(contents), 1
        elif compression == 'raw':
            stored, kind = contents, 0
        else:
            stored, kind = contents, int(compression)
        off = len(f)
        f.extend(stored + bytes([kind]) + struct.pack('<I', mask(crc32c(stored + bytes([kind])))))
        return varint(off) + varint(len(stored))

    index, cur, cur_bytes = [], [], 0
    for key, value in entries:
        cur.append((key, value))
        cur_bytes += len(key) + len(value) + 3
        if cur_bytes >= block_size:
            index.append((cur[-1][0], put_block(build_block(cur, restart_interval))))
            cur, cur_bytes = [], 0
    if cur:
        index.append((cur[-1][0], put_block(build_block(cur, restart_interval))))
    meta = put_block(build_block([], restart_interval))
    idx = put_block(build_block(index, 1))
    footer = meta + idx
    footer += bytes(40 - len(footer)) + struct.pack('<Q', TABLE_MAGIC)
    f.extend(footer)
    with open(path, 'wb') as fh:
        fh.write(bytes(f))
    return len(f)


# ---- the bundle ---------------------------------------------------------------------------------------------------------

class Raw(object):
    """A tensor given as its TF dtype code, shape and stored bytes (bfloat16, strings, deliberately wrong sizes)."""

    def __init__(self, dtype, shape, data):
        self.dtype, self.shape, self.data = dtype, tuple(shape), bytes(data)


def write_bundle(prefix, tensors, num_shards=1, shard_of=None, block_size=4096, restart_interval=16, compression='raw',
                 endianness=0, min_consumer=0, entry_fields=None, skip_shards=()):
    """Write `tensors` {name: ndarray | Raw} as a V2 checkpoint at `prefix`.  `shard_of(name)` picks the data shard (by
    default tensor k goes to shard k % num_shards).  `entry_fields` {name: {field: value}} overrides or adds entry
    fields after they are computed (e.g. {'x': {'size': 3}}, {'x': {'slices': 1}}).  Shards in `skip_shards` are not
    written.  Returns {name: entry message}."""
    M = messages()
    names = sorted(tensors, key=lambda n: n.encode())
    if shard_of is None:
        order = {n: k for k, n in enumerate(names)}
        shard_of = lambda n: order[n] % num_shards      # noqa: E731
    shards = [bytearray() for _ in range(num_shards)]
    entries = {}
    for name in names:
        t = tensors[name]
        if isinstance(t, Raw):
            dtype, shape, data = t.dtype, t.shape, t.data
        else:
            a = np.asarray(t)
            dtype, shape, data = TF_DTYPES[a.dtype], a.shape, a.astype(a.dtype.newbyteorder('<')).tobytes()
        s = shard_of(name)
        e = M['BundleEntryProto']()
        e.dtype = dtype
        for d in shape:
            e.shape.dim.add(size=d)
        e.shard_id = s
        e.offset = len(shards[s])
        e.size = len(data)
        e.crc32c = mask(crc32c(data))
        shards[s] += data
        for field, value in (entry_fields or {}).get(name, {}).items():
            if field == 'slices':
                for _ in range(value):
                    e.slices.add().extent.add(start=0, length=1)
            else:
                setattr(e, field, value)
        entries[name] = e
    h = M['BundleHeaderProto']()
    h.num_shards = num_shards
    h.endianness = endianness
    h.version.producer = 1
    h.version.min_consumer = min_consumer
    table = [(b'', h.SerializeToString())] + [(n.encode(), entries[n].SerializeToString()) for n in names]
    write_table(prefix + '.index', table, block_size=block_size, restart_interval=restart_interval,
                compression=compression)
    for s in range(num_shards):
        if s not in skip_shards:
            with open('%s.data-%05d-of-%05d' % (prefix, s, num_shards), 'wb') as f:
                f.write(bytes(shards[s]))
    return entries


def training_checkpoint(prefix, W, step=0, adam=True, **kw):
    """What a tf.train.Saver of KFNet/train.py holds: the model variables, Adam's two slots per variable,
    beta1_power / beta2_power and an int64 global_step.  Returns {name: entry}."""
    rng = np.random.default_rng(step + 11)
    t = dict(W)
    if adam:
        for k, v in W.items():
            t[k + '/Adam'] = rng.standard_normal(v.shape).astype(np.float32) if v.size < 4096 else np.full(v.shape, 0.5, np.float32)
            t[k + '/Adam_1'] = np.full(v.shape, 0.25, np.float32)
        t['beta1_power'] = np.float32(0.9 ** (step + 1))
        t['beta2_power'] = np.float32(0.999 ** (step + 1))
    t['global_step'] = np.int64(step)
    return write_bundle(prefix, {k: np.asarray(v) for k, v in t.items()}, **kw)
