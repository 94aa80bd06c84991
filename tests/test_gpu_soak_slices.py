"""Seeded slices of the randomised differential soaks (tools/soak_random.py, tools/soak_shards.py, tools/soak_options.py)
inside the driver-run suite (round-4 review, next #8): the soaks found four real bugs in round 4 but only ever ran when the
builder started them.  A FIXED number of seeded cases each (the same cases on every box): random small indices x batch sizes x
damping x plain / accelerated x fixed count / convergence contract x filter outcomes x embedding kinds x engine knobs through
hrag_score_facts / hrag_retrieve / hrag_ppr, and random shard counts x exchange groups through the row-shard entry points,
every case against the oracle.  A failing case prints its parameters: `python tools/soak_random.py --replay '<json>'`
replays it.

The three option slices run the seeded plan of tests/option_helpers.py between them, one per PPR state family (batches <= 8:
the small-batch kernels; 9 .. 64: the fp16 state; >= 65: the e4m3 slabs): random COMPOSED calls -- doc filter in every form,
filter_scope="seeds", group_agg, group_hits, fusion, mmr_*, lexical, boost -- on every entry, each held bit for bit to the
one numpy restatement of the whole call (option_helpers.expected_outputs); every slice boosts calls on all five entries.  tests/test_option_helpers_host.py asserts, without
a GPU, what that plan covers; `python tools/soak_options.py --replay '<json>'` replays a failing call."""

import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_seeded_slice_of_the_random_soak(gpu_device, capsys):
    out = os.path.join(ROOT, "gpurun_out", "test_reports", "soak_random_slice.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    rc = _tool("soak_random").main(["--seconds", "150", "--cases", "160", "--seed", "50501", "--out", out])
    text = capsys.readouterr().out
    assert rc == 0 and "SOAK OK" in text, text[-3000:]


def test_seeded_slice_of_the_shard_soak(gpu_device, capsys):
    out = os.path.join(ROOT, "gpurun_out", "test_reports", "soak_shards_slice.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    rc = _tool("soak_shards").main(["--seconds", "150", "--cases", "200", "--seed", "50502", "--out", out])
    text = capsys.readouterr().out
    assert rc == 0 and "SOAK OK" in text, text[-3000:]


def _option_slice(name, batches, capsys, tmp_path):
    import json
    from tests.helpers import write_test_report
    from tests.option_helpers import ENTRIES, PLAN_CALLS, PLAN_CASES, PLAN_SEED
    out = tmp_path / "calls.json"
    rc = _tool("soak_options").main(["--seconds", "150", "--cases", str(PLAN_CASES), "--calls", str(PLAN_CALLS), "--seed",
                                     str(PLAN_SEED), "--batches", batches, "--out", str(out)])
    text = capsys.readouterr().out
    write_test_report(f"soak_options_{name}_slice", json.loads(out.read_text()))     # with the other slices' reports
    capsys.readouterr()
    assert rc == 0 and "SOAK OK" in text, text[-3000:]
    assert f"{PLAN_CASES // 7 * len(batches.split(','))} cases" in text        # (the time bound did not cut the slice short)
    report = json.loads(out.read_text())
    assert report["boosted"] * 4 >= len(report["calls"]) and set(report["boosted_entries"]) == set(ENTRIES), report["boosted"]
    assert set(report["boosted_batches"]) == {int(x) for x in batches.split(",")}


def test_seeded_slice_of_the_option_soak_small_batches(gpu_device, capsys, tmp_path):
    _option_slice("small", "1,8", capsys, tmp_path)


def test_seeded_slice_of_the_option_soak_fp16_state(gpu_device, capsys, tmp_path):
    _option_slice("fp16", "9,64", capsys, tmp_path)


def test_seeded_slice_of_the_option_soak_e4m3_state(gpu_device, capsys, tmp_path):
    _option_slice("e4m3", "65,130,257", capsys, tmp_path)
