"""The VQA score on the device (meant_vqa_score_update, meant_amd.vqa_score) against an exact host computation: the prediction by
torch.argmax on the CPU (lowest index on a tie, a NaN above everything), the weight there through round(w * 2**32) in Python
integers.  Every counter is an integer, so the state is compared bit for bit."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WEIGHTS = np.array([0.3, 0.6, 0.9, 1.0], dtype=np.float32)     # utils/custom_datasets.py:214-218
SHAPES = [(1, 1), (5, 2), (37, 17), (130, 3129), (9, 64001)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make_case(B, C, dtype, seed, bad_weights=True):
    """scores (rounded to `dtype`, held as float32) and float32 weights.  Per row 0-4 answer columns; in about half of the rows the
    greatest score is put on an answer column (random scores alone almost never land on one), a quarter of those as an exact tie
    of two answer columns and a lower non-answer column where the row has them; some rows carry a NaN score; with bad_weights a few
    predicted weights are inf, NaN, -0.1 and 16.5"""
    rs = np.random.RandomState(seed)
    s = torch.from_numpy(rs.standard_normal((B, C)).astype(np.float32)).to(dtype).float().numpy()
    t = np.zeros((B, C), dtype=np.float32)
    for b in range(B):
        k = min(rs.randint(0, 5), C)
        cols = rs.choice(C, size=k, replace=False)
        t[b, cols] = WEIGHTS[rs.randint(0, 4, size=k)]
        if k and rs.rand() < 0.5:
            s[b, cols[0]] = 8.0
            if k > 1 and rs.rand() < 0.5:
                s[b, cols[1]] = 8.0                                # a tie: the lower index decides
        if C > 3 and rs.rand() < 0.15:
            s[b, rs.randint(0, C)] = np.nan                        # ranks above everything, the first one wins
    if bad_weights and B >= 30:
        pred = torch.argmax(torch.from_numpy(s), dim=1).numpy()
        for b, w in zip(range(3, B, max(1, B // 9)), (np.inf, -0.1, 16.5, np.nan, -np.inf, 16.0, 0.0)):
            t[b, pred[b]] = w
    return torch.from_numpy(s), torch.from_numpy(t)


def want_state(scores, weights):
    """[sum_fx, rows, nan rows, invalid rows] in Python integers"""
    pred = torch.argmax(scores, dim=1)
    fx = rows = nan = invalid = 0
    for b in range(scores.shape[0]):
        w = float(weights[b, pred[b]].item())
        nan += int(torch.isnan(scores[b]).any().item())
        if math.isfinite(w) and 0.0 <= w <= 16.0:
            fx += round(w * 2 ** 32)
            rows += 1
        else:
            invalid += 1
    return [fx, rows, nan, invalid]


@pytest.mark.parametrize("tdtype", [torch.float32, torch.bfloat16], ids=["t_f32", "t_bf16"])
@pytest.mark.parametrize("sdtype", [torch.float32, torch.bfloat16], ids=["s_f32", "s_bf16"])
@pytest.mark.parametrize("B,C", SHAPES, ids=[f"{b}x{c}" for b, c in SHAPES])
def test_state_matches_the_host(dev, B, C, sdtype, tdtype):
    from meant_amd import _lib, vqa_score
    s, t = make_case(B, C, sdtype, seed=B + C)
    t = t.to(tdtype).float()                                       # the weights the kernel reads
    want = want_state(s, t)
    if B >= 30:
        assert want[1] > 0 and want[3] >= 4 and want[2] > 0 and want[0] > 0          # every kind of row occurs
    for lds, ldt in ((C, C), (C + 8 - C % 8, C + 3), (C + 1, C + 8 - C % 8)):       # rows on and off the 16-byte grid
        sb = torch.full((B + 1, lds), float("nan"), device=dev, dtype=sdtype)
        tb = torch.full((B + 1, ldt), 5.0, device=dev, dtype=tdtype)
        sb[:B, :C] = s.to(dev)
        tb[:B, :C] = t.to(dev)
        m = vqa_score("val")
        _lib.route_reset()
        m.update(sb[:B, :C], tb[:B, :C])
        assert _lib.route_count("vqa_score") == 1
        assert m.state.cpu().tolist() == want, (lds, ldt, m.state.cpu().tolist(), want)
        assert m.nan_rows() == want[2] and m.invalid_rows() == want[3]
        ref = want[0] / 2 ** 32 / want[1] if want[1] else 0.0
        assert abs(m.compute().item() - ref) <= 1e-15 and m.compute().dtype == torch.float64


def test_float16_and_float64_inputs_and_cpu_tensors(dev):
    """float16 / float64 go through float32 on the device, CPU tensors are moved there"""
    from meant_amd import vqa_score
    s, t = make_case(37, 17, torch.float16, seed=4)
    want = want_state(s, t)
    for sd, td in ((torch.float16, torch.float64), (torch.float64, torch.float16)):
        tt = t.to(td)
        m = vqa_score()
        m.update(s.to(sd), tt)                                     # both on the CPU
        assert m.state.is_cuda and m.state.cpu().tolist() == want_state(s, tt.float())
        m2 = vqa_score(device=dev)
        m2.update(s.to(sd).to(dev), tt)                            # the target alone on the CPU
        assert torch.equal(m2.state, m.state)
    assert want[1] > 0


def test_batching_and_merge_give_the_same_bits(dev, capsys):
    from meant_amd import _lib, vqa_score
    B, C = 130, 3129
    s, t = make_case(B, C, torch.float32, seed=9)
    s, t = s.to(dev), t.to(dev)
    one = vqa_score("all")
    one.update(s, t)
    parts = vqa_score("parts")
    _lib.route_reset()
    at = 0
    for n in (1, 64, 65):
        parts.update(s[at:at + n], t[at:at + n])
        at += n
    parts.update(s[:0], t[:0])                                     # an empty batch: nothing happens
    assert at == B and _lib.route_count("vqa_score") == 3
    a, b = vqa_score("a"), vqa_score("b")
    a.update(s[:77], t[:77])
    b.update(s[77:], t[77:])
    assert a.merge(b) is a
    want = want_state(s.cpu(), t.cpu())
    for m in (one, parts, a):
        assert m.state.cpu().tolist() == want
    assert vqa_score().merge(one).state.cpu().tolist() == want     # merge into an object that never saw a batch
    shown = one.show()
    assert shown.item() == one.compute().item() and "all VQA score" in capsys.readouterr().out
    one.reset()
    assert one.state.cpu().tolist() == [0, 0, 0, 0] and one.compute().item() == 0.0


def test_evaluate_and_metric_group(dev):
    import meant_amd
    from meant_amd import _lib, metric_group, vqa_score
    from meant_amd.train import evaluate
    torch.manual_seed(0)
    model = meant_amd.meant_vqa(128, 128, 4, 32, 32, 16, 1, 7, torch.nn.Embedding(100, 128), num_heads=2).to(dev)
    model.compute_dtype = torch.bfloat16
    rs = np.random.RandomState(2)
    batches = []
    for B in (4, 3):
        ids = torch.from_numpy(rs.randint(0, 100, (B, 16)).astype("int64")).to(dev)
        img = torch.from_numpy(rs.standard_normal((B, 4, 32, 32)).astype("float32")).to(dev)
        _, soft = make_case(B, 7, torch.float32, seed=B, bad_weights=False)
        batches.append((ids, img, torch.ones(B, 16, device=dev), soft))             # the target stays on the CPU, as a loader hands it over
    _lib.route_reset()
    m = evaluate(model, batches, vqa_score("val"))
    assert model.training and _lib.route_count("vqa_score") == 2
    model.eval()
    with torch.no_grad():
        outs = [model(*b[:3]).float().cpu() for b in batches]
    want = want_state(torch.cat(outs), torch.cat([b[3] for b in batches]))
    assert m.state.cpu().tolist() == want and want[1] == 7
    group = metric_group(vqa_score("a"), vqa_score("b"))
    evaluate(model, batches, group)
    assert all(g.state.cpu().tolist() == want for g in group.metrics)
    assert len(group.show()) == 2
    group.reset()
    assert all(g.state.cpu().tolist() == [0, 0, 0, 0] for g in group.metrics)
