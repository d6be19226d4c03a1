"""``Main.py --shortlist`` / ``--shortlist-min-rating``: the flag combinations the parser refuses and the relation index the
rating threshold stands for.  Host only: every refusal happens before anything touches a device."""
import pytest

import helpers  # noqa: F401  (puts the repository root on sys.path)
import Main


@pytest.mark.parametrize('argv, message', [
    (['--shortlist', '50'], '--shortlist shortens the candidate lists'),
    (['--shortlist', '50', '--explain', '3', '--explain-links', 'x.txt'], '--shortlist shortens the candidate lists'),
    (['--shortlist', '50', '--rank-eval', '5', '--rank-negatives', '99'], '--shortlist and --rank-negatives exclude one another'),
    (['--shortlist', '0', '--recommend', '5'], '--shortlist takes M in'),
    (['--shortlist', str(2 ** 31), '--recommend', '5'], '--shortlist takes M in'),
    (['--shortlist-min-rating', '4', '--recommend', '5'], '--shortlist-min-rating names the ratings'),
])
def test_flag_combinations_are_refused(argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        Main.main(argv)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_accepted_combinations_have_no_error():
    assert Main.shortlist_flag_error(None, None, None, False) is None
    assert Main.shortlist_flag_error(200, None, None, 10) is None
    assert Main.shortlist_flag_error(200, 3.5, None, '5,10') is None
    assert Main.shortlist_flag_error(2 ** 31 - 1, None, None, True) is None


def test_the_rating_threshold_is_the_index_of_the_smallest_class_value_at_or_above_it():
    half = [0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0]
    assert Main.shortlist_min_rel([1, 2, 3, 4, 5], None) == 0
    assert Main.shortlist_min_rel([1, 2, 3, 4, 5], 1) == 0
    assert Main.shortlist_min_rel([1, 2, 3, 4, 5], 3.5) == 3
    assert Main.shortlist_min_rel([1, 2, 3, 4, 5], 4) == 3
    assert Main.shortlist_min_rel(half, 4) == 7
    assert Main.shortlist_min_rel(half, 0) == 0
    assert Main.shortlist_min_rel([1, 2, 3, 4, 5], 5.5) == 5          # above every rating: nothing counts
