"""CPU-side checks of generate.py --decode_slots: the flag, its range, and the way it reaches the generator (the inference
configuration that ModelInitializeTask builds, read by InferenceTask.execute: the route of --kv_cache and --share_prompt)."""
import importlib.util
import os
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli():
    spec = importlib.util.spec_from_file_location("commu_cli_generate_slots", os.path.join(ROOT, "commu-code_amd", "generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _margs(cli, *flags):
    return cli.parse_args()["model_args"].parse_known_args(["--checkpoint_dir", "x.pt", "--output_dir", "o", *flags])[0]


def test_the_flag_is_listed_and_defaults_to_64():
    cli = _cli()
    text = cli.parse_args()["model_args"].format_help()
    assert "--decode_slots" in text and "1 .. 256" in text and "64" in text
    margs = _margs(cli)
    assert cli.check_decode_slots(margs) == 64 and margs.decode_slots == 64
    # a namespace from before the flag existed means the default too
    assert cli.check_decode_slots(types.SimpleNamespace()) == 64


@pytest.mark.parametrize("value", ["0", "257", "-3", "12.5", "many", ""])
def test_values_outside_the_range_are_refused_with_the_range_in_the_message(value):
    cli = _cli()
    with pytest.raises(ValueError, match=r"--decode_slots: an integer in \[1, 256\]"):
        cli.check_decode_slots(_margs(cli, "--decode_slots", value))


def test_main_refuses_before_a_model_is_loaded(tmp_path):
    """main() checks the flag first: with a checkpoint path that does not exist the error is the flag's, not the file's."""
    cli = _cli()
    margs = _margs(cli, "--decode_slots", "257")
    iargs = cli.parse_args()["input_args"].parse_known_args(["--output_dir", str(tmp_path), "--num_generate", "1"])[0]
    with pytest.raises(ValueError, match=r"\[1, 256\]"):
        cli.main(margs, iargs)
    assert not os.path.exists(os.path.join(str(tmp_path), "sequences.json"))


@pytest.mark.parametrize("value", [1, 65, 128, 256])
def test_the_value_reaches_the_inference_configuration(value):
    from commu_amd.midi_generator.model_initializer import ModelInitializeTask
    cli = _cli()
    margs = _margs(cli, "--decode_slots", str(value))
    assert cli.check_decode_slots(margs) == value and margs.decode_slots == value and isinstance(margs.decode_slots, int)
    cfg = ModelInitializeTask(margs).inference_cfg
    assert cfg.GENERATION.decode_slots == value


def test_without_the_flag_the_configuration_is_what_it_was():
    from commu_amd.midi_generator.model_initializer import ModelInitializeTask
    cli = _cli()
    margs = _margs(cli)
    cli.check_decode_slots(margs)
    for args in (margs, types.SimpleNamespace(checkpoint_dir="x.pt")):
        cfg = ModelInitializeTask(args).inference_cfg
        assert "decode_slots" not in cfg.GENERATION and getattr(cfg.GENERATION, "decode_slots", 64) == 64


def test_the_pipeline_takes_the_number_of_slots():
    import inspect

    from commu_amd.midi_generator.generate_pipeline import TokenGenerationPipeline
    assert inspect.signature(TokenGenerationPipeline.__init__).parameters["decode_slots"].default == 64
