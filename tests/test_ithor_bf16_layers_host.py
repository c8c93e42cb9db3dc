"""CPU-only checks of tests/ithor_bf16_layers_cpu.py, the float64 layer reference of tests/test_gpu_ithor_bf16_layers.py:
(1) bf16_round is torch's bfloat16 cast and the kernels' integer formula (dense16::bf16_bits) on ties both ways, negatives,
subnormals, the largest finite values and representable values; (2) with rounding switched off every row is ithor_layers_cpu's row,
and on pre-rounded arrays the rounded and the unrounded rows agree, both exactly; (3) fault injection: torch fp32 stands in for the
device at B = 3, h = 84, a fault is put where a kernel would leave it, everything behind it is computed from the faulted buffer,
and EXACTLY the faulted row fails."""
import numpy as np
import pytest
import torch

from oracle.torch_oracle import ithor_seeded
from tests import ithor_bf16_layers_cpu as bl
from tests import ithor_layers_cpu as lc
from tests.ithor_bf16_layers_cpu import bf16_round as q
from tests.test_ithor_layers_host import inputs


# ---- the rounding ---------------------------------------------------------------------------------------------------------------
def bits_formula(x):
    """dense16::bf16_bits / gru_bf16.hip:43 on numpy uint32: (u + 0x7fff + ((u >> 16) & 1)) >> 16, widened back to fp32."""
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff
    return (r << 16).astype(np.uint32).view(np.float32)


def test_bf16_round_is_nearest_even_as_torch_and_as_the_kernels_compute_it():
    f = lambda u: np.array(u, dtype=np.uint32).view(np.float32)      # noqa: E731
    special = f([0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000,       # exact ties: down to even, up to even, and negative
                 0x3f807fff, 0x3f808001, 0x3f80ffff, 0x3f810000,       # either side of a tie, representable
                 0x00000001, 0x00008000, 0x00018000, 0x0000ffff, 0x007fffff, 0x80008001, 0x00800000,      # subnormals
                 0x7f7f0000, 0x7f7e8000, 0x7f7e7fff, 0xff7f0000, 0x7f7effff,      # the largest finite bf16 and its neighbours
                 0x00000000, 0x80000000, 0x3f800000, 0xc0490000])
    rng = np.random.default_rng(1)
    x = np.concatenate([special, (rng.standard_normal(4096) * 10.0 ** rng.integers(-30, 30, 4096)).astype(np.float32),
                        rng.integers(0, 0x7f7f0000, 4096, dtype=np.uint32).view(np.float32)])
    assert np.isfinite(x).all()
    t = torch.from_numpy(x.copy())
    got = q(t)
    assert got.dtype == torch.float32
    assert torch.equal(got, t.to(torch.bfloat16).float())
    assert np.array_equal(got.numpy().view(np.uint32), bits_formula(x).view(np.uint32))
    assert torch.equal(q(t.double()), got.double()) and q(t.double()).dtype == torch.float64
    assert torch.equal(q(got), got)                              # idempotent: a copy of the bf16 copy is the bf16 copy
    s = q(torch.from_numpy(special.copy())).numpy().view(np.uint32)
    assert list(s[:4]) == [0x3f800000, 0x3f820000, 0xbf800000, 0xbf820000]
    assert s[8] == 0 and s[9] == 0 and s[10] == 0x00020000           # subnormal ties go to even too
    assert s[16] == 0x7f7e0000 and s[19] == 0x7f7f0000


def trunc(t):
    """Rounding toward zero: the fault of a kernel that drops the low 16 bits."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(t.dtype)


# ---- the stand-in ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stand_in():
    """torch fp32 as the device: every buffer of a forward and backward of the rounded model at h = 84, B = 3 (6 clips), and the
    result of every row on it."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    P = {k: v.detach() for k, v in ithor_seeded(31).named_parameters()}
    image, snd, g_i, g_s = inputs(84, 3, 91, u8=True)
    inp = (image, snd, g_i.float(), g_s.float())
    b = bl.chain(P, *inp)
    return P, inp, b, bl.check_layers(b, P)


def failing(res):
    return {n for n, (_k, r) in res.items() if not all(x <= 1 for _e, _d, x in r)}


def behind(stand_in, **changed):
    """The rows' results with `changed` buffers in place and everything behind them computed from them; rows none of whose inputs
    and outputs moved keep their result (the same computation on the same bits)."""
    P, inp, b, res = stand_in
    b2, _ = bl.rerun(P, *inp, b, changed)
    t0, t1 = bl.layer_table(b, P), bl.layer_table(b2, P)
    assert [r[0] for r in t0] == [r[0] for r in t1]
    moved = {r1[0] for r0, r1 in zip(t0, t1)
             if not all(torch.equal(x, y) for x, y in zip(r0[3] + r0[4], r1[3] + r1[4]) if torch.is_tensor(x))}
    out = dict(res)
    out.update(bl.check_layers(b2, P, only=lambda n: n in moved))
    return out, moved, b2


def test_the_unfaulted_stand_in_passes_every_row(stand_in):
    _P, _inp, _b, res = stand_in
    assert len(res) == 62 and not failing(res), failing(res)
    assert {"conv fwd", "conv dgrad", "conv wgrad", "conv bgrad", "pool fwd", "pool+relu bwd", "linear fwd", "linear bwd",
            "gru step fwd", "gru gates bwd", "gru wgrad", "gru dgrad", "gru concat", "l2norm fwd", "l2norm bwd"} == {k for k, _ in res.values()}
    assert set(bl.ORDER) <= set(res)


def test_with_rounding_off_every_row_is_the_fp32_checkers_row(stand_in):
    P, _inp, b, _res = stand_in
    mine, theirs = bl.layer_table(b, P, q=bl.ident), lc.layer_table(b, P)
    assert [(r[0], r[1]) for r in mine] == [(r[0], r[1]) for r in theirs] and len(mine) == 62
    for (name, _k, f0, i0, o0), (_n, _k1, f1, i1, o1) in zip(mine, theirs):
        assert all(x is y or torch.equal(x, y) for x, y in zip(i0 + o0, i1 + o1)), name
        for dt in (torch.float32, torch.float64):
            ins = [lc._cast(x, dt) for x in i0]
            for x, y in zip(lc._tuple(f0(*ins)), lc._tuple(f1(*ins))):
                assert torch.equal(x, y), (name, dt)


def test_on_pre_rounded_arrays_rounding_changes_nothing(stand_in):
    """gru.bwd takes the following step's dgh from the buffers in both evaluations (teacher=True): the unrounded row of
    ithor_layers_cpu takes its own, which no rounding of the inputs can make equal."""
    P, _inp, b, _res = stand_in
    rb = {k: (q(v) if v.is_floating_point() else q(v.float() / 255)) for k, v in b.items()}
    rP = {k: q(v) for k, v in P.items()}
    on, off = bl.layer_table(rb, rP, teacher=True), bl.layer_table(rb, rP, q=bl.ident, teacher=True)
    assert len(on) == len(off) == 62
    for (name, _k, f0, i0, _o), (_n, _k1, f1, _i, _o1) in zip(on, off):
        for dt in (torch.float32, torch.float64):
            ins = [lc._cast(x, dt) for x in i0]
            for x, y in zip(lc._tuple(f0(*ins)), lc._tuple(f1(*ins))):
                assert torch.equal(x, y), (name, dt)


def test_the_accumulation_order_emulations_are_the_same_products(stand_in):
    """chunk_dot and the three ORDER emulations compute their rows themselves, at fp32 round-off; the bias emulation is the plain
    sum at a clip count that fills more than one 64-clip slice and leaves the last ragged."""
    P, _inp, b, _res = stand_in
    torch.manual_seed(4)
    A, Bm = q(torch.randn(9, 100)), q(torch.randn(100, 7))
    assert lc.rel(bl.chunk_dot(A, Bm), A.double() @ Bm.double()) < 1e-6
    assert torch.equal(bl.chunk_dot(A[:, :16], Bm[:16]), (A[:, :16].double() @ Bm[:16].double()).float())      # one chunk: one rounding
    x, w, c = b["s1"], P["cnn.2.weight"], P["cnn.2.bias"]
    (clips, emu), = bl.snd2_fwd_order(x, w, c).values()
    assert clips == [0, 5] and lc.rel(emu, bl.conv_fwd(x.double(), w.double(), c.double(), "s2")[clips]) < 2e-6
    g, w6 = b["ga6"], P["imgBranch.14.weight"]
    for p5 in (b["p5"], torch.zeros(2, 128, 6, 6)):                                  # 5 x 5 and 6 x 6 maps
        gg = g[:p5.shape[0]]
        (_, emu), = bl.conv6_dgrad_order(gg, w6, p5).values()
        ref = bl.conv_dgrad(gg.double().reshape(-1, 128, 3, 3), w6.double(), "i6", p5.shape)
        assert float(ref.abs().max()) > 0 and lc.rel(emu, ref) < 1e-6
    d = torch.randn(2, 5, 70, 12)
    assert lc.rel(bl._bias_seq(d), d.double().sum((1, 2))) < 1e-6
    assert set(bl.ORDER) == {"snd2.fwd", "conv6.dgrad", "gru.wgrad"}
    assert set(bl.order_for(3, True)) == set(bl.ORDER) and set(bl.order_for(64, True)) == {"snd2.fwd", "gru.wgrad"}
    assert set(bl.order_for(5, False)) == {"snd2.fwd", "conv6.dgrad"}


def test_sixteen_missing_terms_of_conv_6s_data_gradient_are_caught_under_the_emulated_yardstick(stand_in):
    P, _inp, b, _res = stand_in
    g, w6 = q(b["ga6"]).view(-1, 128, 3, 3), q(P["imgBranch.14.weight"])
    # input pixel (2, 2) meets the tap (1, 1) of output pixel (1, 1) alone: k = co; the last 16 output channels that are alive
    live = torch.nonzero(g[0, :, 1, 1])[-16:, 0]
    miss = g[0, live, 1, 1] @ w6[live, :, 1, 1]                                      # (ci)
    ci = int(miss.abs().argmax())
    gp5 = b["gp5"].clone()
    gp5[0, ci, 2, 2] -= miss[ci]
    only_row_fails(stand_in, "conv6.dgrad", gp5=gp5)


# ---- fault injection ------------------------------------------------------------------------------------------------------------
def only_row_fails(stand_in, row, **changed):
    res, moved, b2 = behind(stand_in, **changed)
    assert row in moved
    assert failing(res) == {row}, (row, {n: res[n] for n in failing(res)})
    return res, moved, b2


def test_one_operand_left_unrounded_fails_its_row_alone(stand_in):
    """One of each product kind: convolution forward, data gradient, weight gradient, linear, GRU recurrent product."""
    P, _inp, b, _res = stand_in
    w_ih, w_hh, b_ih, b_hh = lc.rnn_params(P)
    w3, w4 = P["imgBranch.5.weight"], P["imgBranch.8.weight"]
    _, moved, _ = only_row_fails(stand_in, "conv3.fwd", a3=lc.conv_fwd(b["p2"], q(w3), P["imgBranch.5.bias"], "i"))      # x unrounded
    assert {"conv4.fwd", "img_head0.bwd", "conv1.wgrad"} <= moved                   # (everything behind it moved with it)
    only_row_fails(stand_in, "conv4.dgrad", gp3=lc.conv_dgrad(b["ga4"], q(w4), "i", b["p3"].shape))                      # gy unrounded
    only_row_fails(stand_in, "snd2.dgrad",
                   gs1=lc.conv_dgrad(q(b["gs2"]), P["cnn.2.weight"], "s2", b["s1"].shape, mask=b["s1"]))                 # w unrounded
    only_row_fails(stand_in, "snd3.wgrad", **{"G.cnn.4.weight": lc.conv_wgrad(
        q(b["s2"]), b["gs3"], "s3", P["cnn.4.weight"].shape, seq=True)})                                                 # gy unrounded
    only_row_fails(stand_in, "snd_head2.fwd",
                   hid_s2=lc.linear_fwd(b["hid_s1"], q(P["soundTriplet.2.weight"]), P["soundTriplet.2.bias"], True))     # x unrounded
    _, moved, _ = only_row_fails(stand_in, "gru.fwd", hb=bl.gru_unroll(b["gi"], w_hh, b_hh, qh=bl.ident))                # h unrounded
    assert {"gru.bwd", "gru.wgrad", "snd1.wgrad", "snd_head0.fwd"} <= moved


def test_truncation_instead_of_nearest_even_fails_its_row_alone(stand_in):
    P, _inp, b, _res = stand_in
    s2 = lc.conv_fwd(trunc(b["s1"]), trunc(P["cnn.2.weight"]), P["cnn.2.bias"], "s2")
    only_row_fails(stand_in, "snd2.fwd", s2=s2)
    ga = b["ga3"]
    only_row_fails(stand_in, "conv3.wgrad", **{"G.imgBranch.5.weight": lc.conv_wgrad(
        trunc(b["p2"]), trunc(ga), "i", P["imgBranch.5.weight"].shape)})


def test_a_carry_that_takes_the_bf16_copy_of_the_state_fails_gru_fwd_alone(stand_in):
    """The state rounded from the previous step's bf16 copy instead of afresh from the fp32 state is NOT distinguishable: the
    copy is the rounding of that fp32 state and rounding is idempotent (pinned above).  What is distinguishable is the fp32
    state itself being carried from the copy (z h on the rounded h)."""
    P, _inp, b, _res = stand_in
    _w_ih, w_hh, _b_ih, b_hh = lc.rnn_params(P)
    assert torch.equal(bl.gru_unroll(b["gi"], w_hh, b_hh, qh=lambda h: q(q(h))), b["hb"])
    only_row_fails(stand_in, "gru.fwd", hb=bl.gru_unroll(b["gi"], w_hh, b_hh, carry=q))


def test_gru_backward_faults_fail_gru_bwd_alone(stand_in):
    """The other direction's W_hh in the backward product; one step's dgh taken from its neighbour.  (Step 70 of 73: a row's error
    is relative to the output's largest magnitude and the seeded model's gate gradients decay by 1e-5 over a dozen steps back
    from the end of the sequence, so the same fault at step 40 moves nothing above the bound.)"""
    P, _inp, b, _res = stand_in
    _w_ih, w_hh, _b_ih, b_hh = lc.rnn_params(P)
    for kw in (dict(w_back=w_hh.flip(0)), dict(nxt=lambda s: s + 2 if s == 70 else s + 1)):
        dgi, dgh = bl.gru_bwd(b["gsraw"], b["hb"], b["gi"], w_hh, b_hh, **kw)
        _, moved, _ = only_row_fails(stand_in, "gru.bwd", dgi=dgi, dgh=dgh)
        assert {"gru.wgrad", "gru.dgrad", "snd3.dgrad", "snd1.wgrad"} <= moved


def test_the_second_clip_slice_missing_from_the_gru_bias_sums_is_caught():
    """66 clips, the GRU weight-gradient row alone (synthetic gate gradients: the row's inputs are all it reads): b_ih / b_hh
    without the clips from 64 on fail, dW_ih / dW_hh pass."""
    g = torch.Generator().manual_seed(9)
    n = 66
    dgi, dgh = torch.randn(2, n, lc.T, lc.G3, generator=g) * 1e-3, torch.randn(2, lc.T, n, lc.G3, generator=g) * 1e-3
    hb, s3 = torch.tanh(torch.randn(2, lc.T + 1, n, lc.GH, generator=g)), torch.relu(torch.randn(n, lc.T, 64, 7, generator=g))
    out = list(bl.gru_wgrad(dgi, dgh, hb, s3))
    P = {k: v.detach() for k, v in ithor_seeded(31).named_parameters()}
    names = [f"G.rnn.{k}_l0{r}" for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh") for r in lc.RNN]

    def run(o):
        b = dict(dgi=dgi, dgh=dgh, hb=hb, s3=s3)
        b.update({names[2 * i + d]: o[i][d] for i in range(4) for d in range(2)})
        res = bl.check_layers(b, P, only=lambda x: x == "gru.wgrad")
        return [x <= 1 for _e, _d, x in res["gru.wgrad"][1]]

    assert run(out) == [True, True, True, True]
    out[2], out[3] = dgi[:, :64].sum((1, 2)), dgh[:, :, :64].sum((1, 2))
    assert run(out) == [True, True, False, False]


def test_a_dropped_border_tap_in_one_output_row_of_sound_conv_2_fails_snd2_fwd_alone(stand_in):
    P, _inp, b, _res = stand_in
    w = P["cnn.2.weight"].clone()
    w[:, :, 0, 4] = 0
    s2 = b["s2"].clone()
    s2[5, 9, 149] = bl.conv_fwd(b["s1"][5:], w, P["cnn.2.bias"], "s2")[0, 9, 149]
    assert not torch.equal(s2, b["s2"])
    only_row_fails(stand_in, "snd2.fwd", s2=s2)


def test_missing_terms_of_weight_gradients_fail_their_rows_alone(stand_in):
    """The last 16 k-terms (k = (step, clip)) of one dW_hh element; one clip's contribution to a small-linear dW."""
    P, _inp, b, _res = stand_in
    n = b["dgh"].shape[2]
    g, h = q(b["dgh"][1]).reshape(-1, lc.G3)[-16:], q(b["hb"][1, :lc.T]).reshape(-1, lc.GH)[-16:]      # the last 16 of 73 n
    assert g.shape[0] == 16 and n == 6
    miss = g.t() @ h
    el = tuple(int(v) for v in np.unravel_index(int(miss.abs().argmax()), miss.shape))
    G = b["G.rnn.weight_hh_l0_reverse"].clone()
    G[el] -= miss[el]
    res, _, _ = only_row_fails(stand_in, "gru.wgrad", **{"G.rnn.weight_hh_l0_reverse": G})
    assert [x <= 1 for _e, _d, x in res["gru.wgrad"][1]] == [True, False, True, True]
    G = b["G.soundTriplet.2.weight"] - torch.outer(q(b["ghid_s2"][4]), q(b["hid_s1"][4]))
    assert not torch.equal(G, b["G.soundTriplet.2.weight"])
    res, _, _ = only_row_fails(stand_in, "snd_head2.bwd", **{"G.soundTriplet.2.weight": G})
    assert [x <= 1 for _e, _d, x in res["snd_head2.bwd"][1]] == [False, True, True]


def test_negative_clips_at_the_batch_based_offset_fail_the_row_that_wrote_them(stand_in):
    """The rows of the sounds' embeddings start at 3 maxB of a buffer planned for maxB > B.  A head that writes its negative clips
    at the B-based offset leaves, where the reader (and the next kernel) looks, what an earlier call left there."""
    P, _inp, b, _res = stand_in
    B, maxB = 3, 16
    stale = torch.full((9 * maxB,), 0.25)
    raw = stale.clone()
    raw[3 * maxB:3 * maxB + 3 * B] = b["raw_s"][:B].reshape(-1)                  # the positive clips, where they belong
    raw[3 * B + 3 * B:3 * B + 6 * B] = b["raw_s"][B:].reshape(-1)                # the negative ones from 3 B + 3 B, not 3 maxB + 3 B
    raw_s = raw[3 * maxB:3 * maxB + 6 * B].view(2 * B, 3)
    assert torch.equal(raw_s[:B], b["raw_s"][:B]) and not torch.equal(raw_s[B:], b["raw_s"][B:])
    _, moved, _ = only_row_fails(stand_in, "snd_head4.fwd", raw_s=raw_s.clone())
    assert {"snd_l2norm.fwd", "snd_l2norm.bwd", "snd_head4.bwd", "gru.bwd", "snd1.wgrad"} <= moved
