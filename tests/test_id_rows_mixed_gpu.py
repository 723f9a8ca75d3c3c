"""Single process: the id tables' row lists across eager full steps, eager short steps (8 and 5 rows), the recording step, replays and
validation passes (tests/id_rows_cases.py tells the cases and the three checks).

Sequences A, B, C x the fixtures id_d32_N2 / both_fh2 / uimg_pid_fh2 x Trainer(device_state=True, dropout=True) plain, with lazy
tables (default ring; flush_every=3) and with micro_batch=4 (every batch of these sequences has more than 4 rows: full and short
batches alike are stepped in passes, 5 rows as 4 + 1).  Per case a reference run that reads no row list, then two runs against it:
the same steps all eager with the row lists, and the mixed sequence.  One fit() case per variant: an epoch of 7 full batches and an
8-row one, twice, recorded against eager.  The replay guard (check 3) is active in every run that replays.

The micro_batch=4 cases of sequences A and B also hold the second piece of state that crosses a step boundary, the count of
site-header rows the next step's head clears: their full eager step (4 passes) follows replays that follow a short eager step (2
passes), and must clear the rows of all 4 passes the replay used, or the next step's delayed scales are those of stale maxima."""
import pytest
import torch

import id_rows_cases as C
from helpers import build_model, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
VARIANTS = {"plain": {}, "lazy": dict(lazy_tables=True), "lazy_flush3": dict(lazy_tables=dict(flush_every=3)), "micro4": dict(micro_batch=4)}

_CASES = {}


def _case(name):
    if name not in _CASES:
        cfg, g, _, _ = load_case(name)
        assert cfg["d"] == 32 and cfg["n_items"] == 200 and cfg["n_users"] == 50
        _CASES[name] = (cfg, g["sd"])
    return _CASES[name]


_BATCHES = {}


def _batches(name, seq_name):
    """(device batches of the sequence, the validation batch): made once per fixture and sequence, never written."""
    key = (name, seq_name)
    if key not in _BATCHES:
        from segmminterest_amd.synth import make_batch
        cfg = _case(name)[0]
        dev = lambda b: {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()}
        vb = make_batch(C.FULL, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg["n_users"], n_items=cfg["n_items"], seed=77)
        _BATCHES[key] = ([dev(b) for b in C.make_batches(cfg, C.SEQUENCES[seq_name])], dev(vb))
    return _BATCHES[key]


def _trainer(name, variant):
    from segmminterest_amd.trainer import Trainer
    cfg, sd = _case(name)
    model = build_model(cfg)
    model.load_state_dict(sd)
    model = model.to(DEV)
    torch.manual_seed(11)          # (the dropout streams of every run start from the same device-side seed words)
    return Trainer(model, lr=1e-3, device_state=True, dropout=True, **VARIANTS[variant])


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", C.FIXTURES)
@pytest.mark.parametrize("seq_name", list(C.SEQUENCES))
def test_mixed_steps_clear_exactly_the_rows_last_scattered(seq_name, name, variant):
    seq = C.SEQUENCES[seq_name]
    batches, vb = _batches(name, seq_name)
    with C.dense_clears():
        ref = C.run_sequence(_trainer(name, variant), seq, batches, vb, mixed=False)
    assert len(set(ref["losses"])) == len(ref["losses"]) == len(batches)          # (the steps are not copies of one another)
    eager = C.run_sequence(_trainer(name, variant), seq, batches, vb, mixed=False)
    C.same_state(eager, ref, "eager steps with row lists")
    with C.replay_guard() as log:
        tr = _trainer(name, variant)
        mixed = C.run_sequence(tr, seq, batches, vb, mixed=True)
    assert log.count("step") == seq.count("P")          # check 3 saw every replay
    C.same_state(mixed, ref, "sequence %s" % seq_name)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fit_recorded_equals_fit_eager_in_id_mode(variant, tmp_path):
    """7 full batches and an 8-row one per epoch, two epochs, a validation every 3 steps: step 4 records, the 8-row batch is stepped
    eagerly, the second epoch opens with a replay behind that eager step.  History, state dict and best checkpoint in every bit."""
    from segmminterest_amd.trainer import CheckPointer
    name = "id_d32_N2"
    cfg = _case(name)[0]
    seq = ["E"] * 7 + ["e8"]
    key = (name, "fit")
    if key not in _BATCHES:
        from segmminterest_amd.synth import make_batch
        dev = lambda b: {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()}
        vbs = [make_batch(C.FULL, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg["n_users"], n_items=cfg["n_items"], seed=s) for s in (100, 101)]
        _BATCHES[key] = ([dev(b) for b in C.make_batches(cfg, seq)], [dev(b) for b in vbs])
    train, valid = _BATCHES[key]
    runs = {}
    for mode in ("eager", "recorded"):
        tr = _trainer(name, variant)
        ck = CheckPointer("main_metric", str(tmp_path / mode), mode="max")
        with C.replay_guard() as log:
            hist = tr.fit(train, valid, epochs=2, valid_step=3, main_metric="NDCG@5", ckpt=ck, permutation=0, recorded=(mode == "recorded"))
        assert log.count("step") == (10 if mode == "recorded" else 0)          # steps 5-7 of epoch 1, 1-7 of epoch 2
        tr.opt.flush_tables()
        torch.cuda.synchronize()
        best = torch.load([str(p) for p in (tmp_path / mode).iterdir() if "best" in p.name][0], map_location="cpu", weights_only=False)
        runs[mode] = (ck, hist, {k: v.detach().clone() for k, v in tr.model.state_dict().items()}, C.snapshot(tr), best)
    (ck_e, h_e, sd_e, sn_e, b_e), (ck_r, h_r, sd_r, sn_r, b_r) = runs["eager"], runs["recorded"]
    assert h_e["global_step"] == h_r["global_step"] == 16
    assert h_e == h_r
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_r[k]), k
    for a, b in zip(sn_e, sn_r):
        assert (a == b).all()
    assert ck_e.best_metric == ck_r.best_metric and b_e["num_epochs"] == b_r["num_epochs"]
    for k in b_e["model"]:
        assert torch.equal(b_e["model"][k], b_r["model"][k]), k
