"""What the distillation functions of tf_fast_rnnt answer to bad arguments before they ask for a device, and which check
answers first when two arguments are bad: rnnt_kd_loss_pruned, rnnt_kd_loss_pruned_factored, rnnt_kd_loss_pruned_topk,
rnnt_loss_pruned_kd, rnnt_loss_pruned_kd_factored, rnnt_kd_topk_teacher and rnnt_node_occupancy_pruned, called with CPU
tensors (B=2, T=4, s_range=2, C=6, S=3; the top-K cache r_t=3, K=2).  The last row of every function is the call with
nothing wrong, which ends in the refusal to run without a device (rnnt_kd_topk_teacher is plain torch and returns).  The
exception types and texts are recorded in tests/golden/kd_python_refusals.json.

    python tests/test_kd_refusals.py        records tests/golden/kd_python_refusals.json from the package as it stands"""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kd_python_refusals.json")

B, T, R, C, S, RT, K = 2, 4, 2, 6, 3, 3, 2


def _x(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def _i(*shape):
    return torch.zeros(*shape, dtype=torch.int32)


def _base(func):
    """the arguments of a call with nothing wrong"""
    if func == "rnnt_kd_topk_teacher":
        return dict(teacher_logits=_x(B, T, RT, C), k=K)
    if func == "rnnt_kd_loss_pruned_topk":
        return dict(logits=_x(B, T, R, C), teacher_values=_x(B, T, RT, K), teacher_indices=_i(B, T, RT, K), ranges=_i(B, T, R),
                    teacher_ranges=_i(B, T, RT))
    args = dict(logits=_x(B, T, R, C), symbols=_i(B, S), ranges=_i(B, T, R), termination_symbol=0)
    if func != "rnnt_node_occupancy_pruned":
        args["teacher_logits"] = _x(B, T, R, C)
    return args


F64, I64 = torch.float64, torch.int64
DENSE = "rnnt_kd_loss_pruned"
FACT = "rnnt_kd_loss_pruned_factored"
TOPK = "rnnt_kd_loss_pruned_topk"
LOSS = "rnnt_loss_pruned_kd"
LFACT = "rnnt_loss_pruned_kd_factored"
TEACH = "rnnt_kd_topk_teacher"
OCC = "rnnt_node_occupancy_pruned"

# (function, label, what replaces or joins the arguments of _base): every check that answers before the device is asked
# for, each on its own; then pairs of two bad arguments; then, last for each function, the call with nothing wrong
CASES = [
    (DENSE, "logits float64", dict(logits=_x(B, T, R, C, dtype=F64))),
    (DENSE, "teacher int64", dict(teacher_logits=torch.zeros(B, T, R, C, dtype=I64))),
    (DENSE, "logits rank 3", dict(logits=_x(B, T, C), teacher_logits=_x(B, T, C))),
    (DENSE, "teacher shape", dict(teacher_logits=_x(B, T, R, C + 1))),
    (DENSE, "mode", dict(mode="half")),
    (DENSE, "temperature 0", dict(temperature=0.0)),
    (DENSE, "temperature inf", dict(temperature=float("inf"))),
    (DENSE, "temperature nan", dict(temperature=float("nan"))),
    (DENSE, "temperature text", dict(temperature="warm")),
    (DENSE, "reduction", dict(reduction="max")),
    (DENSE, "termination_symbol C", dict(termination_symbol=C)),
    (DENSE, "termination_symbol -1", dict(termination_symbol=-1)),
    (DENSE, "pair: logits float64 + temperature 0", dict(logits=_x(B, T, R, C, dtype=F64), temperature=0.0)),
    (DENSE, "pair: mode + reduction", dict(mode="half", reduction="max")),
    (DENSE, "nothing wrong", dict()),

    (FACT, "logits float64", dict(logits=_x(B, T, R, C, dtype=F64))),
    (FACT, "teacher float64", dict(teacher_logits=_x(B, T, R, C, dtype=F64))),
    (FACT, "logits rank 3", dict(logits=_x(B, T, C), teacher_logits=_x(B, T, C))),
    (FACT, "teacher shape", dict(teacher_logits=_x(B, T, R + 1, C))),
    (FACT, "factorization", dict(factorization="rnnt")),
    (FACT, "mode", dict(mode="half")),
    (FACT, "temperature -1", dict(temperature=-1.0)),
    (FACT, "tdt num_durations 0", dict(factorization="tdt")),
    (FACT, "tdt num_durations 6", dict(factorization="tdt", num_durations=6)),
    (FACT, "tdt num_durations == W", dict(factorization="tdt", num_durations=3, logits=_x(B, T, R, 3), teacher_logits=_x(B, T, R, 3))),
    (FACT, "tdt duration_weight -1", dict(factorization="tdt", num_durations=2, duration_weight=-1.0)),
    (FACT, "tdt duration_weight inf", dict(factorization="tdt", num_durations=2, duration_weight=float("inf"))),
    (FACT, "softmax num_durations 2", dict(num_durations=2)),
    (FACT, "hat num_durations 1", dict(factorization="hat", num_durations=1)),
    (FACT, "hat C 1", dict(factorization="hat", logits=_x(B, T, R, 1), teacher_logits=_x(B, T, R, 1))),
    (FACT, "reduction", dict(reduction="max")),
    (FACT, "termination_symbol C", dict(termination_symbol=C)),
    (FACT, "tdt termination_symbol among the durations", dict(factorization="tdt", num_durations=2, termination_symbol=C - 2)),
    (FACT, "node_weights float64", dict(node_weights=_x(B, T, R, dtype=F64))),
    (FACT, "node_weights shape", dict(node_weights=_x(B, T, R + 1))),
    (FACT, "pair: logits float64 + mode", dict(logits=_x(B, T, R, C, dtype=F64), mode="half")),
    (FACT, "pair: temperature 0 + tdt num_durations 0", dict(temperature=0.0, factorization="tdt")),
    (FACT, "pair: node_weights float64 + shape", dict(node_weights=_x(B, T, R + 1, dtype=F64))),
    (FACT, "pair: teacher float64 + logits rank 3", dict(logits=_x(B, T, C), teacher_logits=_x(B, T, C, dtype=F64))),
    (FACT, "pair: teacher shape + factorization", dict(teacher_logits=_x(B, T, R + 1, C), factorization="rnnt")),
    (FACT, "pair: factorization + mode", dict(factorization="rnnt", mode="half")),
    (FACT, "pair: mode + temperature 0", dict(mode="half", temperature=0.0)),
    (FACT, "pair: reduction + termination_symbol C", dict(reduction="max", termination_symbol=C)),
    (FACT, "pair: termination_symbol C + node_weights float64", dict(termination_symbol=C, node_weights=_x(B, T, R, dtype=F64))),
    (FACT, "pair: hat C 1 + reduction", dict(factorization="hat", logits=_x(B, T, R, 1), teacher_logits=_x(B, T, R, 1), reduction="max")),
    (FACT, "pair: softmax num_durations 2 + reduction", dict(num_durations=2, reduction="max")),
    (FACT, "nothing wrong", dict()),
    (FACT, "nothing wrong, tdt with weights", dict(factorization="tdt", num_durations=2, node_weights=_x(B, T, R))),

    (TOPK, "logits float64", dict(logits=_x(B, T, R, C, dtype=F64))),
    (TOPK, "teacher_values float64", dict(teacher_values=_x(B, T, RT, K, dtype=F64))),
    (TOPK, "teacher_indices int64", dict(teacher_indices=torch.zeros(B, T, RT, K, dtype=I64))),
    (TOPK, "teacher_rest float64", dict(teacher_rest=_x(B, T, RT, dtype=F64))),
    (TOPK, "node_weights float16", dict(node_weights=_x(B, T, R, dtype=torch.float16))),
    (TOPK, "logits rank 3", dict(logits=_x(B, T, C))),
    (TOPK, "teacher_values rank 3", dict(teacher_values=_x(B, T, K), teacher_indices=_i(B, T, K))),
    (TOPK, "teacher_values T", dict(teacher_values=_x(B, T + 1, RT, K), teacher_indices=_i(B, T + 1, RT, K))),
    (TOPK, "teacher_values r_t 0", dict(teacher_values=_x(B, T, 0, K), teacher_indices=_i(B, T, 0, K))),
    (TOPK, "K 65", dict(teacher_values=_x(B, T, RT, 65), teacher_indices=_i(B, T, RT, 65))),
    (TOPK, "K 0", dict(teacher_values=_x(B, T, RT, 0), teacher_indices=_i(B, T, RT, 0))),
    (TOPK, "teacher_indices shape", dict(teacher_indices=_i(B, T, RT, K + 1))),
    (TOPK, "no teacher_ranges, r_t 3", dict(teacher_ranges=None)),
    (TOPK, "teacher_ranges shape", dict(teacher_ranges=_i(B, T, RT + 1))),
    (TOPK, "teacher_ranges a list", dict(teacher_ranges=[0])),
    (TOPK, "teacher_rest shape", dict(teacher_rest=_x(B, T, RT + 1))),
    (TOPK, "node_weights shape", dict(node_weights=_x(B, T, R + 1))),
    (TOPK, "temperature 0", dict(temperature=0.0)),
    (TOPK, "reduction", dict(reduction="max")),
    (TOPK, "pair: K 65 + teacher_indices shape", dict(teacher_values=_x(B, T, RT, 65), teacher_indices=_i(B, T, RT, K))),
    (TOPK, "pair: node_weights float16 + logits rank 3", dict(node_weights=_x(B, T, R, dtype=torch.float16), logits=_x(B, T, C))),
    (TOPK, "pair: node_weights shape + temperature 0", dict(node_weights=_x(B, T, R + 1), temperature=0.0)),
    (TOPK, "pair: teacher_ranges shape + teacher_rest shape", dict(teacher_ranges=_i(B, T, RT + 1), teacher_rest=_x(B, T, RT + 1))),
    (TOPK, "pair: temperature 0 + reduction", dict(temperature=0.0, reduction="max")),
    (TOPK, "pair: teacher_rest float64 + node_weights float16",
     dict(teacher_rest=_x(B, T, RT, dtype=F64), node_weights=_x(B, T, R, dtype=torch.float16))),
    (TOPK, "nothing wrong", dict()),
    (TOPK, "nothing wrong, rest and weights", dict(teacher_rest=_x(B, T, RT), node_weights=_x(B, T, R))),

    (LOSS, "rnnt_type", dict(rnnt_type="other")),
    (LOSS, "reduction", dict(reduction="max")),
    (LOSS, "mode: the device is asked for first", dict(mode="half")),
    (LOSS, "temperature 0: the device is asked for first", dict(temperature=0.0)),
    (LOSS, "logits float64: the device is asked for first", dict(logits=_x(B, T, R, C, dtype=F64))),
    (LOSS, "pair: rnnt_type + reduction", dict(rnnt_type="other", reduction="max")),
    (LOSS, "pair: reduction + mode", dict(reduction="max", mode="half")),
    (LOSS, "nothing wrong", dict()),
    (LOSS, "nothing wrong, constrained", dict(rnnt_type="constrained")),

    (LFACT, "rnnt_type", dict(rnnt_type="other")),
    (LFACT, "factorization tdt", dict(factorization="tdt")),
    (LFACT, "factorization", dict(factorization="rnnt")),
    (LFACT, "node_weights text", dict(node_weights="nope")),
    (LFACT, "reduction, hat", dict(factorization="hat", reduction="max")),
    (LFACT, "reduction, softmax", dict(reduction="max")),
    (LFACT, "hat C 1: the device is asked for first", dict(factorization="hat", logits=_x(B, T, R, 1), teacher_logits=_x(B, T, R, 1))),
    (LFACT, "node_weights float64: the device is asked for first", dict(node_weights=_x(B, T, R, dtype=F64))),
    (LFACT, "pair: factorization tdt + node_weights text", dict(factorization="tdt", node_weights="nope")),
    (LFACT, "pair: rnnt_type + factorization", dict(rnnt_type="other", factorization="rnnt")),
    (LFACT, "pair: node_weights text + reduction", dict(node_weights="nope", reduction="max")),
    (LFACT, "pair: hat + temperature 0: the device is asked for first", dict(factorization="hat", temperature=0.0)),
    (LFACT, "nothing wrong", dict()),
    (LFACT, "nothing wrong, hat with occupancy", dict(factorization="hat", node_weights="occupancy")),
    (LFACT, "nothing wrong, weights", dict(node_weights=_x(B, T, R))),

    (TEACH, "k 0", dict(k=0)),
    (TEACH, "k above C", dict(k=C + 1)),
    (TEACH, "k 65", dict(k=65, teacher_logits=_x(B, T, RT, 80))),
    (TEACH, "temperature 0", dict(temperature=0.0)),
    (TEACH, "temperature nan", dict(temperature=float("nan"))),
    (TEACH, "pair: k 0 + temperature 0", dict(k=0, temperature=0.0)),
    (TEACH, "nothing wrong", dict()),

    (OCC, "rnnt_type", dict(rnnt_type="other")),
    (OCC, "factorization tdt", dict(factorization="tdt")),
    (OCC, "factorization", dict(factorization="rnnt")),
    (OCC, "termination_symbol C: the device is asked for first", dict(termination_symbol=C)),
    (OCC, "pair: rnnt_type + factorization tdt", dict(rnnt_type="other", factorization="tdt")),
    (OCC, "nothing wrong", dict()),
]
IDS = [f"{func}: {label}" for func, label, _ in CASES]


def _reply(ft, func, over):
    """[exception type, text] of the call, or [None, "returned"]"""
    try:
        getattr(ft, func)(**{**_base(func), **over})
    except Exception as exc:   # noqa: BLE001  (whatever it is, it is what gets recorded)
        return [type(exc).__name__, str(exc)]
    return [None, "returned"]


def test_the_table_is_the_recorded_one():
    golden = json.load(open(GOLDEN))
    assert len(set(IDS)) == len(IDS) and set(golden) == set(IDS)
    for func in (DENSE, FACT, TOPK, LOSS, LFACT, OCC):      # every function's last row: nothing wrong, and no device
        last = [i for i in IDS if i.startswith(func + ": ")][-1]
        assert "nothing wrong" in last and golden[last][0] == "RuntimeError" and "no CPU fallback" in golden[last][1], last
    assert golden[f"{TEACH}: nothing wrong"] == [None, "returned"]
    assert sum("pair: " in i for i in IDS) >= 12


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_refusal_is_the_recorded_one(ft, case):
    func, _, over = CASES[case]
    assert _reply(ft, func, over) == json.load(open(GOLDEN))[IDS[case]]


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tf-fast-rnnt_amd"))
    import tf_fast_rnnt
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as fh:
        json.dump({i: _reply(tf_fast_rnnt, func, over) for i, (func, _, over) in zip(IDS, CASES)}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", GOLDEN)
