"""GPU: the kmermatcher's identity records take their polynomial hash from csrc/hip/sd_seqhash.h, which clusthash shares: `sdgpu
kmermatcher` on set G of the kmermatcher vectors still writes the entries the reference's own object code recorded (identical sequences,
and sequences identical under the 13-letter alphabet, are grouped by that record alone)."""
import pytest

import kmmgold
from dbutil import read_db, sdgpu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('tag', kmmgold.runs('G'))
def test_kmermatcher_on_set_g_equals_the_reference(tmp_path, tag):
    p = kmmgold.par(tag)
    seq = kmmgold.write_seq_db(tmp_path, 'G', tag)
    out = str(tmp_path / 'pref')
    sdgpu('kmermatcher', seq, out, '-k', p['k'], '--alph-size', p['alph_size'], '--cov-mode', p['cov_mode'], '-c', p['c'], '--kmer-per-seq-scale',
          p['kmer_per_seq_scale'], '--include-only-extendable', int(p['include_only_extendable']), '--threads', '4', '-v', '0')
    want = kmmgold.entries(tag)
    assert read_db(out) == want
    assert any(text.count(b'\n') > 1 for text in want.values())
