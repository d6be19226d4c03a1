"""``Main.py --pair-shortlist`` / ``--pair-hard-share`` / ``--pair-shortlist-min-rating``: the flag combinations the parser
refuses, the defaults and the pair log's two forms.  Host only: every refusal happens before anything touches a device."""
import pytest

import helpers  # noqa: F401  (puts the repository root on sys.path)
import Main


@pytest.mark.parametrize('argv, message', [
    (['--pair-shortlist', '20'], '--pair-shortlist shapes the negatives of --pair-epochs E: give E'),
    (['--pair-hard-share', '0.5'], '--pair-hard-share shapes the negatives of --pair-epochs E: give E'),
    (['--pair-shortlist-min-rating', '4'], '--pair-shortlist-min-rating shapes the negatives of --pair-epochs E: give E'),
    (['--pair-epochs', '2', '--pair-hard-share', '0.5'], '--pair-hard-share names the share of negatives drawn from --pair-shortlist M'),
    (['--pair-epochs', '2', '--pair-shortlist-min-rating', '4'],
     '--pair-shortlist-min-rating names the ratings that count for --pair-shortlist M'),
    (['--pair-epochs', '2', '--pair-shortlist', '0'], '--pair-shortlist takes M in [1, 2^31)'),
    (['--pair-epochs', '2', '--pair-shortlist', '-3', '--pair-hard-share', '0.5'], '--pair-shortlist takes M in [1, 2^31)'),
    (['--pair-epochs', '2', '--pair-shortlist', str(2 ** 31)], '--pair-shortlist takes M in [1, 2^31)'),
    (['--pair-epochs', '2', '--pair-shortlist', '20', '--pair-hard-share', '-0.1'], '--pair-hard-share takes P in [0, 1]'),
    (['--pair-epochs', '2', '--pair-shortlist', '20', '--pair-hard-share', '1.5'], '--pair-hard-share takes P in [0, 1]'),
    (['--pair-epochs', '2', '--pair-shortlist', '20', '--pair-hard-share', 'nan'], '--pair-hard-share takes P in [0, 1]'),
])
def test_flag_combinations_are_refused(argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        Main.main(argv)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_accepted_combinations_have_no_error():
    assert Main.pair_shortlist_flag_error(None, None, None, None) is None
    assert Main.pair_shortlist_flag_error(3, None, None, None) is None
    assert Main.pair_shortlist_flag_error(3, 20, None, None) is None
    assert Main.pair_shortlist_flag_error(3, 1, 0.0, 1.0) is None
    assert Main.pair_shortlist_flag_error(3, 2 ** 31 - 1, 1.0, None) is None
    # the serving shortlist is a flag of its own: neither needs the other
    assert Main.shortlist_flag_error(None, None, None, False) is None
    assert Main.pair_flag_error(3, None, None, None, False, 1) is None


def test_defaults():
    args = Main.build_parser().parse_args([])
    assert (args.pair_shortlist, args.pair_hard_share, args.pair_shortlist_min_rating) == (None, None, None)
    args = Main.build_parser().parse_args(['--pair-epochs', '2', '--pair-shortlist', '20', '--shortlist', '200'])
    assert (args.pair_shortlist, args.shortlist, args.pair_hard_share) == (20, 200, None)


def test_the_pair_log_line_keeps_its_old_form_and_gains_the_kinds():
    old = dict(epoch=2, pair_loss=0.5, mse=1.25, pair_acc=0.75, pairs=8, void=0, steps=1, seconds=0.1)
    assert Main.pair_log_line(old) == 'Pair epoch 2, pair loss 0.500000, mse 1.250000, pair acc 0.750000\n'
    new = dict(old, hard_pairs=2, pair_acc_hard=0.5, pair_acc_uniform=0.875, stale=False)
    assert Main.pair_log_line(new) == ('Pair epoch 2, pair loss 0.500000, mse 1.250000, pair acc 0.750000, hard 0.250000, '
                                       'pair acc hard 0.500000, uniform 0.875000\n')
