"""``--new-ratings``: the file parser and the flag's argument errors (igmc_amd/new_ratings.py; host only)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT
from igmc_amd.new_ratings import flag_error, grown_sizes, parse_new_ratings, read_new_ratings

CV = np.array([0.5, 1.0, 2.0, 3.5, 5.0])


def test_good_file_with_comments_and_removals(tmp_path):
    text = '# new ratings\n\n3 7 5\n  4\t9   0.5  # trailing comment\n3 7 0\n#12 12 12\n10 2 3.5\n2 11 1.0\n'
    u, v, r = parse_new_ratings(text.splitlines(), CV)
    assert u.dtype == np.int32 and v.dtype == np.int32 and r.dtype == np.uint8
    assert u.tolist() == [3, 4, 3, 10, 2] and v.tolist() == [7, 9, 7, 2, 11]
    assert r.tolist() == [5, 1, 0, 4, 2]          # index in class_values + 1; 0 removes; the order of the lines is kept
    path = tmp_path / 'new.txt'
    path.write_text(text)
    for a, b in zip(read_new_ratings(str(path), CV), (u, v, r)):
        assert np.array_equal(a, b)
    e = parse_new_ratings(['# nothing', '   '], CV)
    assert [len(x) for x in e] == [0, 0, 0] and e[2].dtype == np.uint8


def test_integer_class_values_accept_both_spellings():
    u, v, r = parse_new_ratings(['0 0 4', '0 1 4.0'], np.arange(1, 6))
    assert r.tolist() == [4, 4]


@pytest.mark.parametrize('bad, needle', [('1 2 4', 'rating 4'), ('1 2 abc', 'not a number'), ('1 2', 'expected'),
                                         ('1 2 3 4', 'expected'), ('x 2 5', 'integer ids'), ('-1 2 5', 'ids must be'),
                                         ('1 %d 5' % (2 ** 31 - 1), 'ids must be')])
def test_bad_line_is_named(bad, needle):
    with pytest.raises(ValueError) as e:
        parse_new_ratings(['# c', '0 0 5', '', bad, '1 1 5'], CV, name='f.txt')
    assert 'f.txt, line 4' in str(e.value) and needle in str(e.value)


def test_ids_beyond_the_graph_grow_it():
    u, v, r = parse_new_ratings(['40 3 5', '2 99 1.0', '1 1 0'], CV)
    assert grown_sizes(30, 60, u, v) == (41, 100)
    assert grown_sizes(50, 200, u, v) == (50, 200)
    assert grown_sizes(5, 6, u[:0], v[:0]) == (5, 6)


def test_flag_errors():
    assert flag_error(None, 0, None, True) is None
    assert flag_error('f', 3, None, False) is None and flag_error('f', 0, '5,10', False) is None
    assert '--recommend' in flag_error('f', 0, None, False)
    assert '--use-features' in flag_error('f', 3, None, True)


def test_main_refuses_the_flag_alone_and_with_features(tmp_path):
    """The command line itself: an argparse error (exit status 2) before any data is read."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for extra, needle in ((['--new-ratings', 'f.txt'], '--recommend'),
                          (['--new-ratings', 'f.txt', '--recommend', '3', '--use-features'], '--use-features')):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'Main.py')] + extra, cwd=str(tmp_path), env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        out = r.stdout.decode()
        assert r.returncode == 2 and 'error:' in out and needle in out, out[-2000:]
        assert not os.listdir(str(tmp_path))          # nothing was created: the refusal comes first
