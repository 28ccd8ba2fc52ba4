"""The shipped configuration files of the reference (VERDICT r4 #2c): config.from_yaml on launch/config/config_sim.yaml and
config2.yaml must give exactly the presets the GPU parity tests run (SDEF = CONFIG_SIM_YAML, CONFIG2_YAML), and the older
files that lack the current keys must be refused like the reference refuses them (yaml-cpp throws, yamlRead.h:25-48).
tests/golden/reference_yaml_params.json holds the two current files' parsed values (tools/make_yaml_fixture.py); the YAML
files the loader reads here are written from it, in the layout of the shipped files."""
import dataclasses
import json
import os

import pytest

from mlmapping_amd import config as C

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_yaml_params.json")
# the keys the three older shipped files (config.yaml, d435i_mit_flvis.yaml, l515_t265.yaml) all lack: the sub-box map, the
# camera intrinsics, the depth noise model and the inflation keys that the current reference reads at init (mlmap.cpp:75)
OLDER_FILES_LACK = ("mlmapping_apply_inflate", "mlmapping_cam_cx", "mlmapping_cam_cy", "mlmapping_cam_fx", "mlmapping_cam_fy",
                    "mlmapping_depth_noise_coe", "mlmapping_inflate_global_n", "mlmapping_inflate_n", "mlmapping_subbox_d_xyz",
                    "mlmapping_subbox_n")


def _yaml_value(v):
    if isinstance(v, bool):
        return "true" if v else "false"
    s = repr(v)
    return s.replace("e", ".0e") if isinstance(v, float) and "e" in s and "." not in s else s  # (YAML 1.1 floats need a dot)


def _write_config(path, params):
    """`params` as a config file of the reference: `key: value` lines with trailing comments, and T_B_S as the flow sequence
    yaml-cpp accepts and strict loaders do not — its rows from column 0 of the lines after the key (config_sim.yaml:51-55)."""
    lines = ["# written from tests/golden/reference_yaml_params.json"]
    lines += [f"{k}: {_yaml_value(v)}   # {k}" for k, v in params.items() if k != "T_B_S"]
    m = [_yaml_value(float(v)) for v in params["T_B_S"]]
    rows = [", ".join(m[4 * r:4 * r + 4]) for r in range(4)]
    lines += ["T_B_S:", "[" + rows[0] + ",  # row 0", rows[1] + ",", rows[2] + ",", rows[3] + "]"]
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def _same(a, b):
    assert dataclasses.asdict(a) == dataclasses.asdict(b)


def test_fixture_params_equal_presets():
    y = json.load(open(GOLD))
    _same(C.from_params(y["config_sim.yaml"], 640, 360), C.CONFIG_SIM_YAML)
    _same(C.from_params(y["config_sim.yaml"], 640, 360), C.SDEF)
    _same(C.from_params(y["config2.yaml"], 424, 240), C.CONFIG2_YAML)
    assert C.CONFIG2_YAML.use_exploration_frontiers and C.CONFIG2_YAML.apply_inflate and C.CONFIG2_YAML.cam_cx == 212.6516265869


def test_from_yaml_on_the_reference_files(tmp_path):
    gold = json.load(open(GOLD))
    sim = _write_config(tmp_path / "config_sim.yaml", gold["config_sim.yaml"])
    c2 = _write_config(tmp_path / "config2.yaml", gold["config2.yaml"])
    assert open(sim).read().count("\n[") == 1  # (T_B_S starts in column 0: the loader has to indent it)
    _same(C.from_yaml(sim), C.SDEF)            # 2 * round(cx) x 2 * round(cy) = 640 x 360
    _same(C.from_yaml(c2, 424, 240), C.CONFIG2_YAML)
    auto = C.from_yaml(c2)
    assert (auto.width, auto.height) == (426, 234)
    for name, want in gold.items():  # the loader reads back every value of the file, T_B_S included
        y = C.load_reference_yaml(str(tmp_path / name))
        assert {k: y[k] for k in want} == want
    # the three older files cannot be loaded by the current reference (mlmap.cpp:75 reads mlmapping_subbox_d_xyz): refused here too
    for name in ("config.yaml", "d435i_mit_flvis.yaml", "l515_t265.yaml"):
        old = _write_config(tmp_path / name, {k: v for k, v in gold["config2.yaml"].items() if k not in OLDER_FILES_LACK})
        with pytest.raises(KeyError, match="mlmapping_"):
            C.from_yaml(old)


def test_c_struct_carries_every_key():
    c = C.to_c(C.CONFIG2_YAML)
    assert (c.am_d_rho, c.am_n_rho, c.use_exploration_frontiers, c.apply_inflate, c.inflate_n, c.inflate_global_n, c.sample_cnt) == (0.2, 40, 1, 1, 2, 2, 500)
    assert (c.cam_cx, c.cam_cy, c.cam_fx, c.cam_fy, c.depth_noise_coe, c.occupied_sh) == (212.6516265869, 117.238, 213.728866577, 213.728866577, 0.00375, 2.0)
    assert list(c.T_bs) == C.T_BS_SIM
