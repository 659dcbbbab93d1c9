"""bench.py's options: a plain run (the driver's `--gpus 1 --steps N --warmup W`) leaves the side measurements out; `--full` asks for them."""
import bench


def test_full_is_off_by_default():
    assert bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"]).full is False
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--no-e2e"])
    assert a.full is True and a.no_e2e is True and a.steps == 20 and a.warmup == 5
