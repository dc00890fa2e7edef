"""Reading TensorFlow V2 checkpoints without TensorFlow (kfnet_amd/checkpoint.py, the library's kfn_crc32c), on the CPU.

The files are written by tests/tf_bundle_writer.py: protobuf messages from google.protobuf with descriptors built there,
tables from a LevelDB-style builder -- an encoder independent of the reader under test."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

pytest.importorskip('google.protobuf')

import tf_bundle_writer as TW  # noqa: E402
from kfnet_amd import checkpoint as CK  # noqa: E402
from kfnet_amd.checkpoint import CheckpointError  # noqa: E402
from kfnet_amd.tools.io import get_snapshot  # noqa: E402
from kfnet_amd.weights import load_npz, load_snapshot, synthetic_weights, variable_specs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bitwise_crc32c(data, crc=0):
    c = crc ^ 0xffffffff
    for b in bytes(data):
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 & -(c & 1))
    return c ^ 0xffffffff


# ---- CRC-32C ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('data,want', [(bytes(32), 0x8A9136AA), (b'\xff' * 32, 0x62A8AB43),
                                       (bytes(range(32)), 0x46DD794E), (bytes(range(31, -1, -1)), 0x113FDB5C),
                                       (b'123456789', 0xE3069283)])
def test_crc32c_known_answers(data, want):
    """RFC 3720 B.4 and the customary check value."""
    assert bitwise_crc32c(data) == want
    assert CK.crc32c(data) == want


def test_crc32c_matches_bitwise_on_every_length_and_in_chunks():
    rng = np.random.default_rng(3)
    buf = rng.integers(0, 256, 200, dtype=np.uint8).tobytes()
    for n in range(65):
        for off in (0, 1, 3, 7):      # every alignment of the start
            piece = buf[off:off + n]
            assert CK.crc32c(piece) == bitwise_crc32c(piece), (n, off)
    big = rng.integers(0, 256, (3 << 20) + 5, dtype=np.uint8).tobytes()
    want = CK.crc32c(big)
    c = 0
    for lo, hi in ((0, 1), (1, 9), (9, 1000), (1000, 1 << 20), (1 << 20, len(big))):
        c = CK.crc32c(big[lo:hi], c)
    assert c == want
    assert CK.crc32c(big[:4096]) == bitwise_crc32c(big[:4096])
    assert CK.crc32c(b'') == 0 and CK.crc32c(b'', 0x1234) == 0x1234


def test_crc32c_table_and_sse42_paths_agree(tmp_path):
    """kfn_ckpt.hip is host code that a plain C++ compiler builds: compile it with a driver that runs BOTH
    implementations (the library runs only the one cpuid selects) over every length, alignment and split."""
    if shutil.which('g++') is None:
        pytest.skip('needs g++')
    drv = tmp_path / 'drv.cpp'
    drv.write_text(r'''
#include <cstdarg>
#include <cstdio>
#include "kfn_ckpt.hip"
namespace kfn { int fail(int code, const char*, ...) { return code; } }
int main() {
  static unsigned char buf[1 << 16];
  uint32_t s = 12345;
  for (auto& b : buf) { s = s * 1103515245u + 12345u; b = (unsigned char)(s >> 16); }
  if (!have_sse42()) { std::printf("table-only 0 e3069283\n"); return 0; }
  long bad = 0;
  for (size_t off = 0; off < 8; ++off)
    for (size_t n = 0; n < 300; ++n) {
      const uint32_t a = crc32c_table(~0u, buf + off, n), b = crc32c_sse42(~0u, buf + off, n);
      bad += a != b;
    }
  uint32_t a = crc32c_table(~0u, buf, sizeof buf), b = crc32c_sse42(~0u, buf + 0, 777);
  b = crc32c_sse42(b, buf + 777, sizeof buf - 777);
  bad += a != b;
  uint32_t c = 0;
  kfn_crc32c("123456789", 9, &c);
  std::printf("%ld %08x\n", bad, c);
  return 0;
}
''')
    exe = tmp_path / 'drv'
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-x', 'c++', '-I', os.path.join(ROOT, 'kfnet_amd', 'csrc'),
                           str(drv), '-o', str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert out[-2:] == ['0', 'e3069283'], out


def test_mask_unmask():
    rng = np.random.default_rng(0)
    for c in [0, 1, 0xffffffff, 0xa282ead8] + [int(x) for x in rng.integers(0, 1 << 32, 100, dtype=np.uint64)]:
        assert CK.unmask(CK.mask(c)) == c
        assert CK.mask(c) == TW.mask(c)
    assert CK.mask(0) == 0xa282ead8


# ---- snappy -------------------------------------------------------------------------------------------------------------

def test_snappy_every_tag_kind():
    lit = bytes(range(256)) * 3
    s = TW.varint(0)
    assert CK.snappy_decompress(s) == b''
    # short literal, literals with 1..4 extended length bytes (60..63)
    for n in (1, 60, 61, 300, 70000):
        data = (lit * (n // len(lit) + 1))[:n]
        assert CK.snappy_decompress(TW.varint(n) + TW.snappy_literal(data)) == data
    for k in (1, 2, 3, 4):
        n = 1 << (8 * (k - 1)) if k > 1 else 61
        data = bytes(np.random.default_rng(k).integers(0, 256, n, dtype=np.uint8))
        stream = TW.varint(n) + bytes([(59 + k) << 2]) + (n - 1).to_bytes(k, 'little') + data
        assert CK.snappy_decompress(stream) == data
    # copies: 1-, 2-, 4-byte offsets
    base = bytes(range(100))
    for width, ln in ((1, 4), (1, 11), (2, 1), (2, 64), (4, 33)):
        stream = TW.varint(100 + ln) + TW.snappy_literal(base) + TW.snappy_copy(90, ln, width)
        assert CK.snappy_decompress(stream) == base + (base[10:] * 2)[:ln]


def test_snappy_long_offsets_and_overlapping_copies():
    # a run: 'ab' then a copy of offset 2 and length 40 (overlaps itself)
    stream = TW.varint(42) + TW.snappy_literal(b'ab') + TW.snappy_copy(2, 40, 2)
    assert CK.snappy_decompress(stream) == b'ab' * 21
    stream = TW.varint(12) + TW.snappy_literal(b'x') + TW.snappy_copy(1, 11, 1)
    assert CK.snappy_decompress(stream) == b'x' * 12
    # an offset past 64 KiB needs the 4-byte form
    head = bytes(np.random.default_rng(1).integers(0, 256, 70000, dtype=np.uint8))
    stream = TW.varint(70010) + TW.snappy_literal(head) + TW.snappy_copy(70000, 10, 4)
    assert CK.snappy_decompress(stream) == head + head[:10]
    # the test compressor's output round-trips
    rng = np.random.default_rng(2)
    for data in (b'', b'abc', bytes(5000), b'hello world ' * 400,
                 bytes(rng.integers(0, 4, 100000, dtype=np.uint8)), bytes(rng.integers(0, 256, 3000, dtype=np.uint8))):
        assert CK.snappy_decompress(TW.snappy_compress(data)) == data


@pytest.mark.parametrize('stream', [
    TW.varint(5) + TW.snappy_literal(b'ab') + bytes([1 | (0 << 2), 0]),          # copy offset 0
    TW.varint(10) + TW.snappy_literal(b'ab') + TW.snappy_copy(3, 4, 1),            # offset past the output
    TW.varint(10) + TW.snappy_literal(b'abcd'),                                   # output shorter than declared
    TW.varint(3) + TW.snappy_literal(b'abcd'),                                    # longer than declared
    TW.varint(10) + bytes([9 << 2]) + b'abc',                                     # literal past the input
    TW.varint(10) + TW.snappy_literal(b'ab') + bytes([2]),                        # truncated copy
    TW.varint(100) + bytes([62 << 2, 1]),                                         # truncated literal length
    b'\xff\xff\xff\xff\xff\xff',                                                  # bad length varint
])
def test_snappy_refuses_malformed_streams(stream):
    with pytest.raises(CheckpointError):
        CK.snappy_decompress(stream)


# ---- the table ----------------------------------------------------------------------------------------------------------

def _entries(n=500):
    rng = np.random.default_rng(n)
    keys = sorted({('scope/layer%03d/%s' % (i // 3, 'kernel/Adam' if i % 3 == 1 else 'bias')).encode() + bytes([i % 7])
                   for i in range(n)})
    return [(k, bytes(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8))) for k in keys]


@pytest.mark.parametrize('compression', ['raw', 'snappy'])
@pytest.mark.parametrize('block_size,restart', [(64, 1), (256, 4), (4096, 16), (1 << 20, 1000)])
def test_table_roundtrip(tmp_path, compression, block_size, restart):
    ents = _entries()
    p = str(tmp_path / 't.index')
    TW.write_table(p, ents, block_size=block_size, restart_interval=restart, compression=compression)
    assert CK.read_table(p) == ents


def _corrupt(path, pos, xor=0x01):
    b = bytearray(open(path, 'rb').read())
    b[pos] ^= xor
    open(path, 'wb').write(bytes(b))


def test_table_refuses_corruption(tmp_path):
    ents = _entries(200)
    p = str(tmp_path / 't.index')
    size = TW.write_table(p, ents, block_size=128, restart_interval=2, compression='snappy')
    good = open(p, 'rb').read()
    # a flipped byte anywhere in the blocks (data, trailer, metaindex, index) is a CRC error
    for pos in range(0, size - 48, max(1, (size - 48) // 97)):
        open(p, 'wb').write(good)
        _corrupt(p, pos)
        with pytest.raises(CheckpointError, match='CRC-32C mismatch|compression type|runs past'):
            CK.read_table(p)
    open(p, 'wb').write(good)
    _corrupt(p, size - 1)
    with pytest.raises(CheckpointError, match='magic'):
        CK.read_table(p)
    for cut in (10, 48, size // 2, size - 1):
        open(p, 'wb').write(good[:cut])
        with pytest.raises(CheckpointError):
            CK.read_table(p)


def test_table_refuses_keys_out_of_order_and_unknown_compression(tmp_path):
    p = str(tmp_path / 't.index')
    ents = _entries(50)
    TW.write_table(p, ents[:20] + [ents[30]] + ents[20:30], block_size=100, check_order=False)
    with pytest.raises(CheckpointError, match='out of order'):
        CK.read_table(p)
    TW.write_table(p, ents[:3] + ents[2:3], check_order=False)
    with pytest.raises(CheckpointError, match='out of order'):
        CK.read_table(p)
    TW.write_table(p, ents, compression=2)
    with pytest.raises(CheckpointError, match=r't\.index.*compression type 2'):
        CK.read_table(p)


# ---- the bundle ---------------------------------------------------------------------------------------------------------

def _mixed_tensors():
    rng = np.random.default_rng(5)
    t = {'f32': rng.standard_normal((3, 4)).astype(np.float32), 'f64': rng.standard_normal(5),
         'i32': rng.integers(-9, 9, (2, 2, 2)).astype(np.int32), 'u8': rng.integers(0, 255, 7).astype(np.uint8),
         'i16': np.array([-3, 300], np.int16), 'i8': np.array([[-1, 2]], np.int8), 'i64': np.int64(-(1 << 40)),
         'b': np.array([True, False, True]), 'f16': rng.standard_normal(9).astype(np.float16),
         'scalar': np.float32(2.5), 'empty': np.zeros((0, 3), np.float32)}
    return t


@pytest.mark.parametrize('num_shards,compression', [(1, 'raw'), (3, 'snappy'), (3, 'raw')])
def test_bundle_every_dtype(tmp_path, num_shards, compression):
    t = _mixed_tensors()
    bf = np.array([1.5, -2.0, 3.140625], np.float32)
    t_all = dict(t, bf16=TW.Raw(TW.DT_BFLOAT16, (3,), (bf.view(np.uint32) >> 16).astype('<u2').tobytes()))
    prefix = str(tmp_path / 'model.ckpt-7')
    ents = TW.write_bundle(prefix, t_all, num_shards=num_shards, compression=compression, block_size=64,
                           restart_interval=2)
    # proto3 leaves zero fields off the wire: the first tensor of shard 0 has neither shard_id nor offset
    assert any(e.shard_id == 0 and e.offset == 0 for e in ents.values())
    ck = CK.Checkpoint(prefix)
    assert ck.names() == sorted(t_all)
    for k, v in t.items():
        v = np.asarray(v)
        got = ck.read(k)
        assert got.dtype == v.dtype and got.shape == v.shape and np.array_equal(got, v), k
        assert ck.shape(k) == v.shape and ck.dtype(k) == str(v.dtype if v.dtype != np.bool_ else 'bool')
    assert ck.dtype('bf16') == 'bfloat16' and ck.read('bf16').dtype == np.float32
    assert np.array_equal(ck.read('bf16'), bf)
    assert ck.shape('scalar') == () and ck.read('scalar').shape == ()
    if num_shards == 3:
        assert sorted({e.shard_id for e in ents.values()}) == [0, 1, 2]
        assert os.path.exists(prefix + '.data-00002-of-00003')


def _simple(tmp_path, **kw):
    prefix = str(tmp_path / 'model.ckpt-1')
    t = {'a': np.arange(6, dtype=np.float32).reshape(2, 3), 'b': np.ones(4, np.float32)}
    t.update(kw.pop('extra', {}))
    TW.write_bundle(prefix, t, **kw)
    return prefix


def test_bundle_refusals(tmp_path):
    with pytest.raises(CheckpointError, match='big-endian'):
        CK.Checkpoint(_simple(tmp_path, endianness=1))
    with pytest.raises(CheckpointError, match='version'):
        CK.Checkpoint(_simple(tmp_path, min_consumer=2))
    ck = CK.Checkpoint(_simple(tmp_path, entry_fields={'a': {'slices': 2}}))
    with pytest.raises(CheckpointError, match='a is a partitioned variable'):
        ck.read('a')
    assert np.array_equal(ck.read('b'), np.ones(4, np.float32))
    ck = CK.Checkpoint(_simple(tmp_path, extra={'s': TW.Raw(TW.DT_STRING, (1,), b'\x03abc')}))
    assert ck.dtype('s') == 'string'
    with pytest.raises(CheckpointError, match='s has dtype string'):
        ck.read('s')
    ck = CK.Checkpoint(_simple(tmp_path, entry_fields={'a': {'size': 20}}))
    with pytest.raises(CheckpointError, match='a holds 20 bytes'):
        ck.read('a')
    prefix = _simple(tmp_path, num_shards=2, skip_shards=(1,))
    ck = CK.Checkpoint(prefix)
    with pytest.raises(CheckpointError, match=r'data-00001-of-00002 is missing'):
        ck.read('b')
    assert ck.read('a').shape == (2, 3)
    # a flipped byte in the data: the error names the variable and the file
    prefix = _simple(tmp_path)
    _corrupt(prefix + '.data-00000-of-00001', 24 + 5)
    ck = CK.Checkpoint(prefix)
    assert ck.read('a').shape == (2, 3)
    with pytest.raises(CheckpointError, match=r'variable b \(data file .*model\.ckpt-1\.data-00000-of-00001'):
        ck.read('b')
    # a truncated data file
    prefix = _simple(tmp_path)
    with open(prefix + '.data-00000-of-00001', 'r+b') as f:
        f.truncate(30)
    with pytest.raises(CheckpointError, match='truncated'):
        CK.Checkpoint(prefix).read('b')
    # V1 (one file) and missing checkpoints
    v1 = tmp_path / 'model.ckpt-5'
    v1.write_bytes(b'\0' * 64)
    with pytest.raises(CheckpointError, match='V1'):
        CK.Checkpoint(str(v1))
    with pytest.raises(CheckpointError, match='missing'):
        CK.Checkpoint(str(tmp_path / 'nothing'))


# ---- load_checkpoint ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def full_ckpt(tmp_path_factory):
    """Full architecture (24.4 M + 0.7 M parameters), Adam slots, beta powers, int64 global_step, snappy index."""
    d = tmp_path_factory.mktemp('full')
    W = synthetic_weights(99)
    prefix = str(d / 'model.ckpt-2500')
    ents = TW.training_checkpoint(prefix, W, step=2500, compression='snappy', block_size=1024)
    return prefix, W, ents


def test_load_checkpoint_equals_the_written_weights(full_ckpt):
    prefix, W, _ = full_ckpt
    ck = CK.Checkpoint(prefix)
    assert ck.dtype('global_step') == 'int64' and ck.read('global_step') == 2500
    assert len(ck.names()) == 3 * len(W) + 3
    got, ck = CK.restore(prefix)
    assert list(got) == list(W)
    for k in W:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], W[k]), k
    assert ck.timings['bytes'] == 4 * sum(v.size for v in W.values())       # the Adam slots were not read
    only = CK.load_checkpoint(prefix, scopes=('Temporal',))
    assert sorted(only) == sorted(k for k in W if k.startswith('Temporal/'))


def test_adam_bytes_are_never_read(tmp_path):
    W = {k: v for k, v in synthetic_weights(3).items() if k.startswith('Temporal/')}
    prefix = str(tmp_path / 'model.ckpt-3')
    ents = TW.training_checkpoint(prefix, W, step=3)
    data = prefix + '.data-00000-of-00001'
    for k, e in ents.items():
        if k.endswith('/Adam') or k.endswith('/Adam_1'):
            _corrupt(data, e.offset + e.size // 2, 0xff)
    got = CK.load_checkpoint(prefix)
    assert sorted(got) == sorted(W) and all(np.array_equal(got[k], W[k]) for k in W)
    with pytest.raises(CheckpointError, match='Adam'):
        CK.Checkpoint(prefix).read('Temporal/fc1/kernel/Adam')


def test_scope_only_and_errors(tmp_path):
    W = synthetic_weights(4)
    sc = {k: v for k, v in W.items() if k.startswith('ScoreNet/')}
    prefix = str(tmp_path / 'model.ckpt-1')
    TW.training_checkpoint(prefix, sc, step=1, adam=False)
    got = CK.load_checkpoint(prefix)
    assert sorted(got) == sorted(sc)
    # the strict engines refuse what is missing; the reader just returns what is there
    part = dict(sc)
    del part['ScoreNet/conv3a/bias']
    prefix = str(tmp_path / 'model.ckpt-2')
    TW.training_checkpoint(prefix, part, step=2, adam=False)
    assert 'ScoreNet/conv3a/bias' not in CK.load_checkpoint(prefix)
    bad = dict(sc, **{'ScoreNet/conv7/kernel': np.zeros((1, 1, 256, 64), np.float32)})
    prefix = str(tmp_path / 'model.ckpt-3')
    TW.training_checkpoint(prefix, bad, step=3, adam=False)
    with pytest.raises(ValueError, match=r'ScoreNet/conv7/kernel has shape \[1, 1, 256, 64\]'):
        CK.load_checkpoint(prefix)
    half = {k: v.astype(np.float16) for k, v in sc.items() if 'conv7' in k or 'prediction' in k}
    prefix = str(tmp_path / 'model.ckpt-4')
    TW.write_bundle(prefix, half)
    got = CK.load_checkpoint(prefix)
    assert all(got[k].dtype == np.float32 and np.array_equal(got[k], half[k].astype(np.float32)) for k in half)
    prefix = str(tmp_path / 'model.ckpt-5')
    TW.write_bundle(prefix, {'Temporal/fc2/bias': np.arange(32, dtype=np.int32)})
    with pytest.raises(ValueError, match='Temporal/fc2/bias has dtype int32'):
        CK.load_checkpoint(prefix)


def test_model_variables_cover_the_specs():
    mv = CK.model_variables()
    assert len(mv) == 2 * len(variable_specs())
    assert mv == {k: v.shape for k, v in synthetic_weights(1).items()}


# ---- get_snapshot, load_snapshot, the CLI -------------------------------------------------------------------------------

def _touch_ckpt(folder, step):
    (folder / ('model.ckpt-%d.index' % step)).write_bytes(b'')
    (folder / ('model.ckpt-%d.data-00000-of-00001' % step)).write_bytes(b'')


def test_get_snapshot_precedence(tmp_path):
    d = tmp_path
    assert get_snapshot(str(d)) == (None, 0)
    _touch_ckpt(d, 100)
    assert get_snapshot(str(d)) == (str(d / 'model.ckpt-100'), 100)
    (d / 'kfnet_weights-99.npz').write_bytes(b'')
    assert get_snapshot(str(d)) == (str(d / 'model.ckpt-100'), 100)
    (d / 'kfnet_weights-100.npz').write_bytes(b'')                    # a tie: the .npz wins
    assert get_snapshot(str(d)) == (str(d / 'kfnet_weights-100.npz'), 100)
    _touch_ckpt(d, 2500)
    _touch_ckpt(d, 900)
    assert get_snapshot(str(d)) == (str(d / 'model.ckpt-2500'), 2500)
    (d / 'kfnet_weights-10000.npz').write_bytes(b'')
    assert get_snapshot(str(d)) == (str(d / 'kfnet_weights-10000.npz'), 10000)
    e = tmp_path / 'only_step0'
    e.mkdir()
    (e / 'kfnet_weights.npz').write_bytes(b'')
    _touch_ckpt(e, 0)
    assert get_snapshot(str(e)) == (str(e / 'kfnet_weights.npz'), 0)
    assert not get_snapshot(str(d))[0].endswith('.index')


def test_load_snapshot_and_cli_roundtrip(tmp_path, capsys):
    W = {k: v for k, v in synthetic_weights(8).items() if k.startswith('Temporal/')}
    prefix = str(tmp_path / 'model.ckpt-40')
    TW.training_checkpoint(prefix, W, step=40, num_shards=2, compression='snappy')
    got = load_snapshot(prefix)
    out = capsys.readouterr().out
    n = len(W)
    assert 'model.ckpt-40 (step 40): %d variables restored, %d ignored' % (n, 2 * n + 3) in out
    assert sorted(got) == sorted(W) and all(np.array_equal(got[k], W[k]) for k in W)
    assert CK.main(['list', prefix]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 3 * n + 3
    assert 'global_step (int64) []' in lines
    assert 'Temporal/fc1/kernel (float32) [128, 64]' in lines
    npz = str(tmp_path / 'kfnet_weights-40.npz')
    assert CK.main(['to-npz', prefix, npz]) == 0
    back = load_npz(npz)
    assert sorted(back) == sorted(W) and all(np.array_equal(back[k], W[k]) for k in W)
    only = str(tmp_path / 'fc.npz')
    assert CK.main(['to-npz', prefix, only, '--scope', 'ScoreNet']) == 0
    assert load_npz(only) == {}
    _corrupt(prefix + '.index', 3)
    capsys.readouterr()
    assert CK.main(['list', prefix]) == 1
    assert 'CRC-32C mismatch' in capsys.readouterr().err


def test_modes_load_weights_reports_a_bad_checkpoint(tmp_path, capsys):
    import argparse
    from kfnet_amd import modes
    W = {k: v for k, v in synthetic_weights(8).items() if k.startswith('Temporal/fc')}
    prefix = str(tmp_path / 'model.ckpt-5')
    ents = TW.write_bundle(prefix, W)
    a = argparse.Namespace(random_weights=False, model_folder=str(tmp_path))
    got = modes.load_weights(a)
    assert sorted(got) == sorted(W)
    e = ents['Temporal/fc2/kernel']
    _corrupt(prefix + '.data-00000-of-00001', e.offset + 7)
    capsys.readouterr()
    assert modes.load_weights(a) is None
    err = capsys.readouterr().err
    assert 'Temporal/fc2/kernel' in err and 'CRC-32C mismatch' in err
    empty = tmp_path / 'empty'
    empty.mkdir()
    assert modes.load_weights(argparse.Namespace(random_weights=False, model_folder=str(empty))) is None
    assert 'kfnet_weights*.npz or model.ckpt-*.index' in capsys.readouterr().out


def test_block_trailer_layout(tmp_path):
    """The footer and trailer as the format describes them: handles, zero padding, magic; type byte + masked CRC."""
    p = str(tmp_path / 't.index')
    TW.write_table(p, [(b'', b'h'), (b'k', b'v')])
    b = open(p, 'rb').read()
    assert struct.unpack('<Q', b[-8:])[0] == CK.TABLE_MAGIC
    off, size, _ = CK._block_handle(b[-48:], 0, 'footer')
    assert b[off + size] == 0 and CK.unmask(struct.unpack('<I', b[off + size + 1:off + size + 5])[0]) == \
        bitwise_crc32c(b[off:off + size + 1])
