"""GPU: rsp_fingerprint (csrc/fingerprint.hip) through rspnet_amd.fingerprint.FingerprintSet against the numpy restatement --
every size at which the kernel takes another path, four alignments, special values, an int64 and an empty tensor -- then address
independence, sensitivity, determinism (two calls, a side stream, capture and replay), the pretext step eager against replayed, and
the fine-tune Engine's NaN halt."""
import random

import numpy as np
import pytest
import torch

import finetune_loop_util as U
from rspnet_amd import fingerprint as F
from test_fingerprint_cpu import case_D, case_E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193, 3 * 8192 + 17)
LONG = 3 * 8192 + 17
NAN_A, NAN_B = 0x7FC00000, 0xFFC12345      # two NaN payloads


def _special(v):
    """±0.0, denormals, ±Inf and two NaN payloads at positions 0, last, 8191 and 8192 (where the segment has them) and their
    neighbours."""
    w = v.view(np.uint32)
    n = w.size
    marks = [(0, NAN_A), (1, 0x80000000), (2, 0x00000001), (n - 1, 0xFF800000), (n - 2, 0x807FFFFF), (8191, 0x7F800000),
             (8190, 0x00000000), (8192, NAN_B), (8193, 0x00400000)]
    for pos, bits in marks:
        if 0 <= pos < n:
            w[pos] = bits
    return v


@pytest.fixture(scope="module")
def case():
    """One buffer, every segment carved from it at 0, 1, 2 and 3 floats past a 16-byte boundary (the same values at the four
    offsets of a size), cases D and E, an int64 tensor and an empty one; the reference records, computed once."""
    rng = np.random.default_rng(20240)
    values = {n: rng.standard_normal(n).astype(np.float32) for n in SIZES}
    for n in SIZES:
        if n > 8192:
            _special(values[n])
    extra = {"D": case_D(), "E": case_E()}
    layout, cursor = [], 0
    for n in SIZES:
        for off in range(4):
            start = (cursor + 3) // 4 * 4 + off
            layout.append((f"n{n}+{off}", start, n, values[n]))
            cursor = start + n
    for k, v in extra.items():
        start = (cursor + 3) // 4 * 4 + 1
        layout.append((k, start, v.size, v))
        cursor = start + v.size
    host = np.zeros(cursor + 8, np.float32)
    for _, start, n, v in layout:
        host[start:start + n] = v
    buf = torch.from_numpy(host).to(DEV)
    assert buf.data_ptr() % 16 == 0
    names = [l[0] for l in layout] + ["int64", "empty"]
    counters = torch.arange(-3, 5000, dtype=torch.int64, device=DEV) * 2654435761
    tensors = [buf[start:start + n] for _, start, n, _ in layout] + [counters, torch.empty(0, device=DEV)]
    host_list = [l[3] for l in layout] + [counters.cpu().numpy(), np.zeros(0, np.float32)]
    ref = F.reference_records(host_list)
    fs = F.FingerprintSet(names, tensors)
    return {"names": names, "tensors": tensors, "host": host_list, "ref": ref, "fs": fs, "buf": buf}


def test_kernel_matches_the_restatement(case):
    """hash, nonfinite and max_abs exactly; sumsq and sum_abs within 1e-9 relative of numpy's float64 sums (recursive summation of
    n <= 2^20 non-negative doubles is within n * 2^-53 = 1.2e-10 of the true sum; the gate sits about 8x above that); D and E, whose
    sums are exact in any order, exactly.  The restatement follows the kernel's summation order, so the whole record is the same
    32 bytes as well."""
    fs, ref = case["fs"], case["ref"]
    assert fs.native and fs.total_chunks == sum(-(-w // 8192) for w in fs.words)
    fs.run()
    got = fs.read()
    worst = 0.0
    for name, g, r, h in zip(case["names"], got, ref, case["host"]):
        assert g["hash"] == r["hash"] and g["nonfinite"] == r["nonfinite"] and g["max_abs"] == r["max_abs"], name
        if h.dtype == np.float32 and h.size:
            w = h.view(np.uint32)
            fin = h[(w & 0x7F800000) != 0x7F800000].astype(np.float64)
            assert g["nonfinite"] == h.size - fin.size and g["max_abs"] == (np.abs(fin).max() if fin.size else 0), name
            for key, want in (("sumsq", np.sum(fin * fin)), ("sum_abs", np.sum(np.abs(fin)))):
                err = abs(g[key] - want) / want if want else abs(g[key])
                worst = max(worst, err)
                assert err <= 1e-9, (name, key, g[key], want)
        else:
            assert (g["sumsq"], g["sum_abs"], g["max_abs"], g["nonfinite"]) == (0.0, 0.0, 0.0, 0), name
    print(f"\nworst relative difference to numpy's float64 sums: {worst:.2e}")
    d, e = got[case["names"].index("D")], got[case["names"].index("E")]
    assert (f"{int(d['hash']):016x}", d["sumsq"], d["sum_abs"], d["max_abs"], d["nonfinite"]) == ("00000ff74603c94b", 108838.171875, 25859.875, 6.25, 0)
    assert (f"{int(e['hash']):016x}", e["sumsq"], e["sum_abs"], e["max_abs"], e["nonfinite"]) == ("00000ff72b6d48a1", 108742.015625, 25841.375, 6.25, 3)
    assert got[case["names"].index("empty")].tobytes() == bytes(32)
    assert got[case["names"].index(f"n{LONG}+0")]["nonfinite"] == 4
    assert got.tobytes() == ref.tobytes()


def test_address_and_alignment_independence(case):
    """The same values at the four offsets past a 16-byte boundary -- float4 loads at offset 0, scalar loads at the others -- and in
    a fresh allocation: byte-identical records, the doubles included."""
    fs = case["fs"]
    fs.run()
    got = fs.read()
    for n in SIZES:
        recs = [got[case["names"].index(f"n{n}+{off}")].tobytes() for off in range(4)]
        assert recs[0] == recs[1] == recs[2] == recs[3], n
    i = case["names"].index(f"n{LONG}+3")
    moved = torch.from_numpy(case["host"][i].copy()).to(DEV)
    other = F.FingerprintSet(["moved"], [moved])
    other.run()
    assert other.read()[0].tobytes() == got[i].tobytes()
    # the same set on tensors that moved: the table follows
    other.run([case["tensors"][i]])
    assert other.read()[0].tobytes() == got[i].tobytes()


def test_sensitivity(case):
    """The lowest mantissa bit of one element, wherever it sits: that tensor's hash changes and no other record does.  A swap of two
    unequal elements changes the hash too (an abs-sum cannot see either)."""
    fs, names = case["fs"], case["names"]
    fs.run()
    base = fs.read()
    i = names.index(f"n{LONG}+1")
    bits = case["tensors"][i].view(torch.int32)
    for pos in (0, 4, 8191, 8192, LONG - 1):
        bits[pos] ^= 1
        fs.run()
        got = fs.read()
        bits[pos] ^= 1
        assert got[i]["hash"] != base[i]["hash"], pos
        same = np.arange(len(names)) != i
        assert got[same].tobytes() == base[same].tobytes(), pos
    j = names.index("n1025+2")
    t = case["tensors"][j]
    a, b = t[7].clone(), t[900].clone()
    assert float(a) != float(b)
    t[7], t[900] = b, a
    fs.run()
    got = fs.read()
    t[7], t[900] = a, b
    assert got[j]["hash"] != base[j]["hash"] and got[j]["max_abs"] == base[j]["max_abs"]
    assert abs(got[j]["sum_abs"] - base[j]["sum_abs"]) <= 1e-12 * base[j]["sum_abs"]
    fs.run()
    assert fs.read().tobytes() == base.tobytes()


def test_determinism_two_calls_a_side_stream_and_replay(case):
    fs = case["fs"]
    first = fs.run()
    second = fs.run()
    assert first.data_ptr() != second.data_ptr() and first.shape == (len(case["names"]), 32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = fs.run()
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(first, second) and torch.equal(first, third)
    assert first.cpu().numpy().tobytes() == case["ref"].tobytes()
    # capture one call (linear, one stream), change the data in place, replay: the records of the NEW data
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rec = fs.run()
    buf = case["buf"]
    saved = buf.clone()
    buf.mul_(-1.5)
    buf[::7] += 0.25
    g.replay()
    torch.cuda.synchronize()
    want = F.reference_records([t.cpu().numpy() for t in case["tensors"]])
    got = rec.cpu().numpy().reshape(-1).view(F.REC_DTYPE)
    buf.copy_(saved)
    assert want.tobytes() != case["ref"].tobytes()
    assert np.array_equal(got["hash"], want["hash"]) and np.array_equal(got["nonfinite"], want["nonfinite"])
    assert np.array_equal(got["max_abs"], want["max_abs"])
    assert got.tobytes() == want.tobytes()
    fs.run()
    assert fs.read().tobytes() == case["ref"].tobytes()


def test_ops_argument_checks():
    from rspnet_amd import _lib, ops
    be = ops.backend()
    table, out = torch.zeros(64, dtype=torch.uint8, device=DEV), torch.zeros(64, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.RspError):
        be.fingerprint(table, 3, 1, out)                                  # three jobs do not fit 64 bytes
    with pytest.raises(_lib.RspError):
        be.fingerprint(table.cpu(), 2, 1, out)
    with pytest.raises(_lib.RspError):
        F.FingerprintSet(["host"], [torch.zeros(4)])                      # no CPU path on the HIP backend
    with pytest.raises(TypeError):
        F.FingerprintSet(["half"], [torch.zeros(4, dtype=torch.float16, device=DEV)])
    assert F.FingerprintSet([], []).run().shape == (0, 32)


def test_pretext_step_eager_and_replayed_leave_the_same_fingerprints():
    """C3D at fixture size, three steps by the five statements and three through GraphedPretextStep(issue="graph") from the same seeds:
    the gradient and the state records of every step are equal, and the eager step's gradient records are those of copies of the
    .grad tensors."""
    from rspnet_amd.graph_step import GraphedPretextStep
    from oracle import portable as P
    from test_graph_step_gpu import _build
    arch, B, HW, K, steps = "c3d", 4, 32, 64, 3
    clips = [tuple(torch.from_numpy(c).to(DEV) for c in P.clips(10 + i, 0, (B, 3, 32, HW, HW))) for i in range(steps)]
    traces = []
    for how in ("eager", "graph"):
        torch.manual_seed(7)
        torch.cuda.manual_seed(7)
        random.seed(7)
        wrapped, crit, opt = _build(arch, K)
        stepper = GraphedPretextStep(wrapped, crit, opt, warmup=2, issue="graph") if how == "graph" else None
        sets, trace = None, []
        for im_q, im_k in clips:
            if stepper is None:
                out, tgt, rl, rt = wrapped(im_q, im_k)
                loss, la, lm = crit(out, tgt, rl, rt)
                opt.zero_grad()
                loss.backward()
                opt.step()
            else:
                stepper(im_q, im_k)
            grads, state = F.named_gradients(wrapped), F.named_state(wrapped)
            if sets is None:
                sets = (F.FingerprintSet(*zip(*grads)), F.FingerprintSet(*zip(*state)))
            trace.append((sets[0].run([t for _, t in grads]), sets[1].run([t for _, t in state])))
            if stepper is None:
                copies = [t.detach().cpu().clone() for _, t in grads]
                assert trace[-1][0].cpu().numpy().tobytes() == F.reference_records(copies).tobytes()
        torch.cuda.synchronize()
        if stepper is not None:
            assert not stepper.disabled and len(stepper.graphs) == 1, stepper.fallback_reason
        traces.append((sets[0].names, sets[1].names, trace))
    (gn0, sn0, te), (gn1, sn1, tg) = traces
    assert gn0 == gn1 and sn0 == sn1 and len(gn0) > 10 and "queue_ptr" in sn0 and "queue" in sn0
    for i, ((g0, s0), (g1, s1)) in enumerate(zip(te, tg)):
        assert torch.equal(g0, g1), ("gradients", i, [gn0[j] for j in (g0 != g1).any(dim=1).nonzero().flatten().tolist()][:8])
        assert torch.equal(s0, s1), ("state", i, [sn0[j] for j in (s0 != s1).any(dim=1).nonzero().flatten().tolist()][:8])
    assert not torch.equal(te[0][0], te[1][0]) and not torch.equal(te[0][1], te[1][1])      # (the steps themselves differ)


def test_finetune_engine_halts_on_a_nonfinite_gradient(tmp_path):
    """A NaN classifier weight (data, not a GPU fault): FloatingPointError naming the tensor between backward and the optimizer;
    every parameter keeps its bits."""
    from rspnet_amd import ops
    from rspnet_amd.finetune import Engine
    assert ops.backend().name == "hip"
    _, meta, state = U.load()
    cfg = dict(U.config(meta), fingerprint={"every": 1, "halt_on_nonfinite": True})
    eng = Engine(U.make_args(tmp_path), cfg, 0, train_loader=U.FixtureLoader(meta, "train", DEV),
                 validate_loader=U.FixtureLoader(meta, "val", DEV))
    eng.model.module.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    with torch.no_grad():
        eng.model.module.fc.weight[0, 0] = float("nan")
    before = {n: p.detach().clone() for n, p in eng.model.module.named_parameters()}
    with pytest.raises(FloatingPointError, match="fc.weight"):
        eng.train_epoch()
    torch.cuda.synchronize()
    for n, p in eng.model.module.named_parameters():
        assert torch.equal(p.detach().view(torch.int32), before[n].view(torch.int32)), n
    assert not (tmp_path / "fingerprints.jsonl").exists()
