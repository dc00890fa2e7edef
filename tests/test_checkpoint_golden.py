"""The checkpoint reader against a file TensorFlow itself wrote: tests/golden/tf1_ckpt/, made by
`python tools/tf1_dump_golden.py --ckpt tests/golden/tf1_ckpt` where TF 1.x exists (a tf.train.Saver V2 checkpoint of four
model variables with Adam slots, beta powers and global_step, and expected.npz of every variable's value).  Skips while
nobody has produced it, as tests/test_golden.py does for tests/golden/tf1_kfnet_*.npz."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FOLDER = os.path.join(HERE, 'golden', 'tf1_ckpt')
EXPECTED = os.path.join(FOLDER, 'expected.npz')


@pytest.mark.skipif(not os.path.exists(EXPECTED), reason='no tests/golden/tf1_ckpt/: nobody has run '
                    'tools/tf1_dump_golden.py --ckpt (the reader is checked against tests/tf_bundle_writer.py only)')
def test_reader_reads_a_tensorflow_written_checkpoint():
    from kfnet_amd import checkpoint as CK
    from kfnet_amd.tools.io import get_snapshot
    prefix, step = get_snapshot(FOLDER)
    assert prefix is not None and not prefix.endswith('.npz') and step >= 1
    ck = CK.Checkpoint(prefix)
    with np.load(EXPECTED) as z:
        want = {k: z[k] for k in z.files}
    assert set(ck.names()) == set(want)
    for k, v in want.items():
        got = ck.read(k)
        assert got.shape == v.shape and np.array_equal(got, v), k
    assert int(ck.read('global_step')) == step
    W = CK.load_checkpoint(prefix)
    assert sorted(W) == sorted(k for k in want if k.split('/')[0] in ('ScoreNet', 'Temporal') and 'Adam' not in k)
    assert all(np.array_equal(W[k], want[k]) for k in W)
