"""``Main.cold_start_flag_error`` / ``Main.cold_start_levels``: the argument checks of ``--cold-start`` / ``--cold-users`` /
``--cold-draw``, as functions of the flags alone (no GPU, no data)."""
import pytest

import helpers  # noqa: F401  (puts the repository root on sys.path)
import Main


@pytest.mark.parametrize('spec,levels', [('1', [1]), ('0', [0]), ('1,2,5,10', [1, 2, 5, 10]), ('10,1', [10, 1]),
                                         ('1,2,3,4,5,6,7,8', [1, 2, 3, 4, 5, 6, 7, 8])])
def test_levels_are_parsed(spec, levels):
    assert Main.cold_start_levels(spec) == levels


@pytest.mark.parametrize('spec', ['', 'a', '1,,2', '1.5', '-1', '1,-2', '1,1', '1,2,3,4,5,6,7,8,9', ',', '1;2'])
def test_malformed_levels_are_refused(spec):
    assert Main.cold_start_levels(spec) is None
    assert '--cold-start takes 1 to 8' in Main.cold_start_flag_error(spec, None, 0, '5,10', None)


def test_refusals_name_what_is_missing():
    assert '--rank-eval' in Main.cold_start_flag_error('1,2', None, 0, None, None)
    assert '--new-ratings' in Main.cold_start_flag_error('1,2', None, 0, '5', 'new.txt')
    assert '--cold-users' in Main.cold_start_flag_error(None, '20', 0, '5', None)
    assert '--cold-users' in Main.cold_start_flag_error(None, 'who.txt', 0, None, None)
    assert '--cold-draw' in Main.cold_start_flag_error(None, None, 3, '5', None)
    assert '--cold-draw takes D >= 0' in Main.cold_start_flag_error('1', None, -1, '5', None)


def test_accepted_combinations_have_no_error():
    assert Main.cold_start_flag_error(None, None, 0, None, None) is None
    assert Main.cold_start_flag_error(None, None, 0, '5,10', 'new.txt') is None
    assert Main.cold_start_flag_error('1,2,5,10', None, 0, '5,10', None) is None
    assert Main.cold_start_flag_error('0', '20', 4, '10', None) is None
    assert Main.cold_start_flag_error('1', 'who.txt', 0, '10', None) is None


def test_the_parser_knows_the_flags_and_main_refuses_before_any_work(capsys):
    args = Main.build_parser().parse_args(['--cold-start', '1,3', '--cold-users', '20', '--cold-draw', '2', '--rank-eval', '5'])
    assert (args.cold_start, args.cold_users, args.cold_draw) == ('1,3', '20', 2)
    defaults = Main.build_parser().parse_args([])
    assert (defaults.cold_start, defaults.cold_users, defaults.cold_draw) == (None, None, 0)
    for argv, word in ((['--cold-start', '1,3'], '--rank-eval'), (['--cold-users', '20', '--rank-eval', '5'], '--cold-start'),
                       (['--cold-start', 'x', '--rank-eval', '5'], '1 to 8')):
        with pytest.raises(SystemExit) as e:
            Main.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
