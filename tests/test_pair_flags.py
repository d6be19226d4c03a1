"""``Main.py --pair-epochs`` / ``--pair-checkpoint`` / ``--pair-lr`` / ``--pair-mse-weight``: the flag combinations the parser
refuses, the defaults and the checkpoint file names.  Host only: every refusal happens before anything touches a device."""
import os

import pytest

import helpers  # noqa: F401  (puts the repository root on sys.path)
import Main


@pytest.mark.parametrize('argv, message', [
    (['--pair-lr', '1e-4'], '--pair-lr names the learning rate of --pair-epochs'),
    (['--pair-mse-weight', '0'], '--pair-mse-weight names the squared-error weight of --pair-epochs'),
    (['--pair-epochs', '3', '--pair-checkpoint', '3'], '--pair-epochs and --pair-checkpoint exclude one another'),
    (['--pair-epochs', '3', '--dgcnn-rs'], 'not with --dgcnn-rs'),
    (['--pair-epochs', '0'], '--pair-epochs takes E >= 1'),
    (['--pair-epochs', '-2', '--pair-lr', '1e-4'], '--pair-epochs takes E >= 1'),
    (['--pair-checkpoint', '0'], '--pair-checkpoint takes E >= 1'),
    (['--pair-epochs', '2', '--pair-lr', '0'], '--pair-lr takes LR > 0'),
    (['--pair-epochs', '2', '--pair-mse-weight', '-1'], '--pair-mse-weight takes A >= 0'),
])
def test_flag_combinations_are_refused(argv, message, capsys):
    with pytest.raises(SystemExit) as e:
        Main.main(argv)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_more_than_one_rank_is_refused(monkeypatch, capsys):
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit) as e:
        Main.main(['--pair-epochs', '2'])
    assert e.value.code == 2 and '--pair-epochs runs on one rank (this job has 2)' in capsys.readouterr().err
    assert Main.pair_flag_error(2, None, None, None, False, 2) is not None
    assert Main.pair_flag_error(None, 5, None, None, False, 2) is None          # serving a pair checkpoint: any number of ranks


def test_accepted_combinations_have_no_error():
    assert Main.pair_flag_error(None, None, None, None, False, 1) is None
    assert Main.pair_flag_error(None, None, None, None, True, 8) is None
    assert Main.pair_flag_error(5, None, None, None, False, 1) is None
    assert Main.pair_flag_error(5, None, 1e-4, 0.0, False, 1) is None
    assert Main.pair_flag_error(None, 5, None, None, False, 1) is None
    assert Main.pair_flag_error(None, 5, None, None, True, 1) is None


def test_defaults_and_file_names():
    args = Main.build_parser().parse_args([])
    assert (args.pair_epochs, args.pair_checkpoint, args.pair_lr, args.pair_mse_weight) == (None, None, None, None)
    assert Main.pair_checkpoint_path('results/x_testmode', 5) == os.path.join('results/x_testmode', 'pair_checkpoint5.pth')
    line = Main.pair_log_line(dict(epoch=2, pair_loss=0.5, mse=1.25, pair_acc=0.75))
    assert line == 'Pair epoch 2, pair loss 0.500000, mse 1.250000, pair acc 0.750000\n'
