"""CPU checks of the fp32 training mode's boundary (csrc/train_f32.hip, model.fp32_training, train.py --parity): the new entry
points are declared, exported and bound; the CLI flag parses; the mode is off by default."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("commu_gemm_f32", "commu_relattn_fwd_f32", "commu_relattn_bwd_f32", "commu_layernorm_fwd_f32", "commu_layernorm_bwd_f32",
       "commu_ce_bwd_f32", "commu_embed_bwd_f32", "commu_dropout_f32")


def test_fp32_training_entry_points_declared_exported_and_bound():
    from commu_amd import _lib
    text = open(os.path.join(ROOT, "include", "commu_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(commu_[a-z0-9_]+)\s*\(", text))
    if not os.path.exists(_lib.LIB_PATH):
        import subprocess
        import sys
        subprocess.check_call([sys.executable, os.path.join(ROOT, "commu-code_amd", "build.py")])
    lib = _lib.load()
    for name in NEW:
        assert name in declared, name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), name


def test_train_cli_parity_flag_parses():
    spec = importlib.util.spec_from_file_location("commu_cli_train_host", os.path.join(ROOT, "commu-code_amd", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args(["--data_dir", "d", "--work_dir", "w", "--parity"]).parity is True
    assert mod.parse_args(["--data_dir", "d", "--work_dir", "w"]).parity is False


def test_fp32_training_is_off_by_default():
    from commu_amd.model.config_helper import get_cfg
    from commu_amd.model.dataset import BaseVocab
    from commu_amd.model.model import MemTransformerLM
    cfg = get_cfg(num_layers=2, num_heads=2, units=64, inner_size=128, tgt_length=16, mem_length=16)
    model = MemTransformerLM(cfg, BaseVocab())
    assert model.fp32_training is False
    assert not getattr(model, "parity_fp32", False)
