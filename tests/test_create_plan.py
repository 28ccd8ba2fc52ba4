"""mlm_plan (mlmapping_amd/csrc/mlm_plan.h): everything mlm_create decides without the device — the constants of MlmDev, LDS sizes,
launch geometries, the tile edge, the sector-path envelope, the frame slots' capacities and the refusals — on the CPU: a stand-alone
driver (tests/cpp/create_plan_driver.cpp) built with g++ -fsanitize=address,undefined, its rows checked here.

* Against tests/golden/create_plan.json: per case the inputs (configuration, limits, knobs, CU count) and what mlm_create of the
  commit BEFORE the plan existed arrived at, dumped at the end of that mlm_create on an MI355X (256 CUs): the scalars of the handle's
  parameter block and of slot 0's, the handle's fields, both capacity sets, the device-memory total and the two MLM_DEBUG_CREATE
  lines; for a refusal the status and mlm_last_error.  The plan reproduces every recorded scalar exactly, except MlmDev::logit_exact
  (the libm of the machine that runs the test) and the device-memory total and second line (they need the allocations:
  tests/test_gpu_geometry.py holds them on the device).
* Invariants over a seeded sweep of random configurations inside the supported envelope, and the one predicate mlm_create's envelope
  and widen_sec_tab share.
"""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "create_plan.json")))["cases"]
MLM_OK, MLM_ERR_INVALID, MLM_ERR_UNSUPPORTED = 0, -1, -4
CAP_MAX = 0xFFFFFFF0
NOT_IN_THE_PLAN = {"P.logit_exact", "h.alloc_bytes"}
# slot 0's copies of the capacities that alloc_slot takes from the handle's caps_now
SLOT_FROM_CAPS = {"S.hl_cap": "hl", "S.mt_cap": "mt", "S.vh_cap": "vh", "S.contrib_cap": "sub", "S.refs_cap": "refs"}
SLOT_FROM_CAPS_TILES = {"S.rec_cap": "rec", "S.sbkt_cap": "sbkt"}  # (allocated with the tiles only: sector path, not frontier mode)


def _statements(case):
    out = [f"case {case['name']}"]
    for k, v in case["cfg"].items():
        out += [f"cfg T_bs {i} {x!r}" for i, x in enumerate(v)] if k == "T_bs" else [f"cfg {k} {v!r}"]
    out += [f"lim {k} {v}" for k, v in case["lim"].items()]
    out += [f"knob {k} {v}" for k, v in case["knobs"].items()]
    out += [f"ncu {case['ncu']}", "run"]
    return out


def _number(text):
    return float(text) if any(c in text for c in ".en") else int(text)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cp") / "create_plan_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "create_plan_driver.cpp"), "-o", str(exe)])

    def run(cases):
        """{case name: {row name: value}} — numbers, but the texts of err and line1 and the number lists of sigma3 / *_lds / widen"""
        text = "\n".join(s for c in cases for s in _statements(c)) + "\n"
        out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout
        plans, cur = {}, None
        for line in out.splitlines():
            key, _, rest = line.partition(" ")
            if key == "case":
                cur = plans.setdefault(rest, {"widen": []})
            elif key == "end":
                cur = None
            elif key in ("err", "line1"):
                cur[key] = rest
            elif key in ("sigma3", "sec_lds", "tile_lds"):
                cur[key] = [_number(x) for x in rest.split()]
            elif key == "widen":
                cur["widen"].append(tuple(int(x) for x in rest.split()))
            else:
                cur[key] = _number(rest)
        assert len(plans) == len(cases)
        return plans

    return run


@pytest.fixture(scope="module")
def golden_plans(plan):
    return plan(GOLDEN)


def test_fixture_holds_the_cases():
    names = {c["name"] for c in GOLDEN}
    assert {"S1", "S1_SIGMA0", "S3", "SDEF", "frontier", "S1_batch8", "S1_batch9", "rho513", "points_2_21", "subbox256", "dmax_gt4",
            "knob_sec_tab_256", "knob_sec_tab_big_0", "knob_sec_threads_512", "knob_tile_sh_1", "knob_bin_block_512", "knob_need_slots_0",
            "knob_sectors_0", "knob_hit_tab_n_0", "knob_slot_sets_2"} <= names
    by = {c["name"]: c for c in GOLDEN}
    v = lambda n, k: by[n]["values"][k]  # noqa: E731
    # the cases are what their names say
    assert (v("S1_batch8", "P.tile_sh"), v("S1_batch9", "P.tile_sh")) == (2, 3)
    assert v("S3", "P.nRho") > 100 and v("S3", "P.sec_tab") == 2048 and v("S3", "h.rank_grid") == 384
    assert all(v(n, "h.use_sectors") == 0 for n in ("rho513", "points_2_21", "subbox256", "knob_sectors_0", "knob_bin_block_512"))
    assert all(v(n, "h.use_sectors") == 1 for n in ("S1", "S3", "SDEF", "frontier"))
    assert v("dmax_gt4", "P.node_lds") == 1024 and v("dmax_gt4", "P.agg_lds") == 512 and v("S1", "P.node_lds") == 448
    assert v("SDEF", "h.no_spread") == 1 and v("S1", "h.no_spread") == 0
    assert v("frontier", "P.explore") == 1 and v("frontier", "h.need_sized") == 0 and v("S1", "h.need_sized") == 1
    assert v("knob_slot_sets_2", "h.n_sets") == 2 and v("knob_hit_tab_n_0", "P.hit_tab_n") == 0 and v("knob_sec_tab_big_0", "P.sec_tab_big") == 0
    refused = {c["err"] for c in GOLDEN if c["status"] != MLM_OK}
    assert len(refused) == 7 and any(c["status"] == MLM_ERR_INVALID and c["err"] == "" for c in GOLDEN)


@pytest.mark.parametrize("case", [c for c in GOLDEN if c["status"] == MLM_OK], ids=lambda c: c["name"])
def test_plan_equals_the_parents_mlm_create(golden_plans, case):
    got, want = golden_plans[case["name"]], case["values"]
    assert got["status"] == MLM_OK and got["err"] == ""
    tiles = bool(got["h.use_sectors"]) and not got["P.explore"]
    checked = 0
    for key, value in want.items():
        if key in NOT_IN_THE_PLAN:
            continue
        if key in SLOT_FROM_CAPS:
            mine = got["caps_now." + SLOT_FROM_CAPS[key]]
        elif key in SLOT_FROM_CAPS_TILES:
            mine = got["caps_now." + SLOT_FROM_CAPS_TILES[key]] if tiles else 0
        elif key == "h.mir.enabled":
            # (mlm_create then applies the limit to the plan's value, mirror_apply_limit: the smallest planes, 256 blocks of
            # 6 bytes per voxel + 13, have to fit max_bytes)
            mine = got[key] and 256 * (got["P.cells"] * 6 + 13) <= got["h.mir.max_bytes"]
        else:
            mine = got[key]
        assert mine == value, (key, mine, value)
        checked += 1
    assert checked == len(want) - len(NOT_IN_THE_PLAN) and checked > 100
    assert got["line1"] + "\n" == case["line1"]


@pytest.mark.parametrize("case", [c for c in GOLDEN if c["status"] != MLM_OK], ids=lambda c: c["name"])
def test_plan_refuses_what_the_parents_mlm_create_refused(golden_plans, case):
    got = golden_plans[case["name"]]
    assert (got["status"], got["err"]) == (case["status"], case["err"])
    assert "P.nRho" not in got


def _random_cases(n, seed):
    rng = np.random.default_rng(seed)
    base = next(c for c in GOLDEN if c["name"] == "S1")
    pick = lambda *a: a[rng.integers(len(a))]  # noqa: E731
    cases = []
    for i in range(n):
        cfg = dict(base["cfg"])
        cfg.update(am_d_rho=pick(0.05, 0.1, 0.2, 0.25), am_d_phi_deg=pick(0.5, 1.0, 2.0, 5.0, 7.5), am_d_z=pick(0.05, 0.1, 0.2, 0.25),
                   am_n_rho=int(pick(rng.integers(2, 40), rng.integers(40, 300), rng.integers(300, 781))), am_n_z_below=int(rng.integers(0, 61)),
                   am_n_z_over=int(rng.integers(0, 61)), depth_noise_coe=pick(1e-6, 0.001, 0.00375, 0.02), subbox_d_xyz=pick(0.05, 0.1, 0.2, 0.4),
                   subbox_n=int(pick(1, 2, 5, 8, 10, 16, 32, 255, 256)), use_exploration_frontiers=int(rng.integers(0, 4) == 0))
        lim = dict(max_blocks=1024, max_points=int(pick(1000, 64 * 48, 640 * 480, 1280 * 720, (1 << 21) - 1, 1 << 21, 3_000_000)),
                   max_batch=int(rng.integers(0, 17)), record_awareness=0)
        knobs = {}
        if rng.integers(0, 3) == 0:
            name, values = pick(("sec_tab", (256, 512, 1024, 2048)), ("sec_threads", (256, 512)), ("bin_block", (256, 512, 1024)), ("need_slots", (0, 1)),
                                ("sectors", (0, 1)), ("slot_sets", (2, 3)), ("hit_tab_n", (0, 64, 1024)))
            knobs[name] = int(pick(*values))
        cases.append(dict(name=f"r{i}", cfg=cfg, lim=lim, knobs=knobs, ncu=256))
    return cases


def _spread_max(sigma3):
    s3, n, dmax = np.asarray(sigma3, dtype=np.float32), len(sigma3), 0
    for r in range(n):
        # centre + (+d, -d) while d < 3 sigma(rho), inside the cylinder, at most MLM_DIFF_RANGE = 10 steps
        reach = [d for d in range(1, 11) if all(np.float32(e) < s3[r] and r + e < n for e in range(1, d + 1))]
        dmax = max(dmax, max(reach, default=0))
    return dmax


def test_invariants_over_random_configurations(plan):
    cases = _random_cases(300, seed=20261019)
    plans = plan(cases)
    accepted = [(c, plans[c["name"]]) for c in cases if plans[c["name"]]["status"] == MLM_OK]
    on_sectors = [(c, p) for c, p in accepted if p["h.use_sectors"]]
    assert len(accepted) > 250 and len(on_sectors) > 60 and sum(1 for _, p in accepted if not p["h.use_sectors"]) > 60
    assert sum(1 for _, p in on_sectors if p["P.explore"]) > 5
    for c, p in accepted:
        why = (c["name"], c["cfg"], c["lim"], c["knobs"])
        tab, edge = p["P.sec_tab"], 1 << p["P.tile_sh"]
        assert tab & (tab - 1) == 0 and tab >= p["h.sec_threads"], why
        assert edge * edge * p["P.lv_nz"] <= 4096, why
        assert p["P.n_tx"] * edge >= p["P.lv_nx"] and (p["P.n_tiles"] // p["P.n_tx"]) * edge >= p["P.lv_ny"] and p["P.n_tiles"] % p["P.n_tx"] == 0, why
        assert p["P.tile_words"] * 32 >= p["P.nPhi"] and p["P.tile_combos"] % 4 == 0, why
        for k in ("hl", "mt", "vh", "rec", "refs", "sub", "sbkt"):
            now, worst = p["caps_now." + k], p["caps_worst." + k]
            assert now <= worst <= CAP_MAX and (p["h.need_sized"] or now == worst), (why, k)
        assert all(p["S." + k] <= CAP_MAX for k in ("nb_cap", "node_cap", "chunk_cap", "mc_cap", "mvox_cap", "touch_cap", "mc_list_cap")), why
        assert p["spread_max"] == _spread_max(p["sigma3"]), why
        assert p["h.no_spread"] == (p["spread_max"] == 0), why
        assert (p["tables.odds"], p["tables.cos_phi"], p["tables.sin_phi"]) == (21 * p["P.nRho"], p["P.nPhi"], p["P.nPhi"]), why
        assert p["tables.sec_const"] == p["P.sec_const_words"] == (21 * p["P.nRho"] + 3) // 4 + (p["P.nRho"] + 3) // 4 * 4, why
    for c, p in on_sectors:
        why = (c["name"], c["cfg"], c["lim"], c["knobs"])
        assert p["P.sec_lds_bytes"] <= 160 * 1024 - 1024 and p["P.sec_big_lds_bytes"] <= 159 * 1024, why
        assert p["h.tile_lds_bytes"] <= 96 * 1024 and p["h.apply_lds_bytes"] <= 150 * 1024, why
        *offs, total, occ = p["sec_lds"]  # tab chunk odds sigma miss rays multi ray_p0 vox aux, in the order they lie in LDS
        assert offs[0] == 0 and offs == sorted(offs) and all(o % 4 == 0 for o in offs) and offs[-1] < total and occ == offs[1], why
        assert total == p["P.sec_lds_bytes"] == p["col_lds"] and offs[-1] + 24 * p["P.nRho"] <= total < offs[-1] + 24 * p["P.nRho"] + 16, why
        *offs, total = p["tile_lds"]  # cnt place desc slot ztab
        assert offs[0] == 0 and offs == sorted(offs) and all(o % 4 == 0 for o in offs) and total == p["h.tile_lds_bytes"], why
        assert offs[-1] + 4 * ((p["P.lv_nz"] + 1) & ~1) <= total < offs[-1] + 4 * ((p["P.lv_nz"] + 1) & ~1) + 16, why
    # widen_sec_tab and mlm_create ask the one predicate: a handle CREATED with the widened table (knob sec_tab) and widen_sec_tab's
    # thread count is on the sector path exactly when the predicate lets widen_sec_tab go there.  (What the two callers add on their
    # own sides: mlm_create the rest of its envelope, which these handles pass and which does not depend on the table; widen_sec_tab
    # its cap of 2048 entries and "smaller than the large table", which only ever keep it from widening.)
    again = []
    for c, p in on_sectors:
        for tab, nt, fits in p["widen"]:
            again.append(dict(c, name=f"{c['name']}_{tab}", knobs=dict(c["knobs"], sec_tab=tab, sec_threads=nt), fits=fits, nt=nt, tab=tab))
    created = plan(again)
    assert sum(c["fits"] for c in again) > 30 and sum(not c["fits"] for c in again) > 30
    for c in again:
        p = created[c["name"]]
        assert (p["P.sec_tab"], p["h.sec_threads"]) == (c["tab"], c["nt"]), c["name"]
        assert bool(p["h.use_sectors"]) == bool(c["fits"]), (c["name"], c["cfg"], c["knobs"])
