"""GPU: the refusals of the C API's MAPPO entry points and of the three resamples on live simulators -- the smallest there are:
Overcooked's cramped_room, Simplecooked's smallest layout and the balance beam at 2 worlds, Cartpole at 1 world as the wrong
game -- held to the whole message and to which check speaks first (tests/capi_refusal_cases.py, tests/golden/capi_refusals.json,
recorded from the library before csrc/capi.hip was split).  Every refused call must also leave the stream empty: every buffer a
launch could write keeps its marks."""
import json

import pytest

pytestmark = pytest.mark.gpu

import capi_refusal_cases as cases  # noqa: E402
from madrona_rl_envs_playground_amd import _lib  # noqa: E402


@pytest.fixture(scope="module")
def live(hip_lib):
    live = cases.Live()
    live.forms = {form.name: form for form in cases.gpu_forms(live)}
    yield live
    live.close()


FORMS = [f"{entry}{where}" for where in (" on overcooked", " on simplecooked")
         for entry in ("mrl_cnn_act", "mrl_cnn_act_bank", "mrl_rollout_cnn", "mrl_rollout_cnn_bank", "mrl_cnn_bank_resample")] + \
        ["mrl_mlpbase_act", "mrl_mlpbase_act_bank", "mrl_rollout_mlpbase", "mrl_rollout_mlpbase_bank", "mrl_mlpbase_bank_resample",
         "mrl_agent_bank_resample"]


def test_every_form_is_run(live):
    assert sorted(live.forms) == sorted(FORMS) == sorted(json.load(open(cases.GOLDEN))["gpu"])


@pytest.mark.parametrize("name", FORMS)
def test_refusals_word_for_word_and_nothing_enqueued(live, name):
    want = cases.expected("gpu", [live.forms[name]])  # (which also holds the number of cases to the file's)
    got = cases.run(_lib.lib(), [live.forms[name]])
    wrong = {case: (got[case], want.get(case)) for case in got if got[case] != want.get(case)}
    assert not wrong, wrong
    assert all(rc != _lib.MRL_OK for rc, _ in got.values()), "every case is a refusal"
    assert live.unchanged(), "a refused call wrote to a record, the ids, the episodes, a workspace, the ring or ACTION"
