"""Plain torch-CPU restatement of the iTHOR actor-critic forward (ai2thorNet_VAR + Categorical's linear layer) from a
state_dict in the reference's layout: the checker of var_amd.IthorNetPolicy for batches the fixture does not hold.
Helper module, not a test file.  Inputs are float tensors already divided by 255 (image (B,3,96,96), occupancy
(B,1,9,9)) on the device the computation should run on; returns value (B,1), actor features (B,128), logits (B,n), rnn_hxs_out (B,1024).
`dtype`: the precision of the whole evaluation (float64: the reference of tests/acting_layers_cpu.py)."""
import torch
import torch.nn.functional as F


def forward(sd, image, occupancy, image_feat, goal_sound_feat, rnn_hxs, masks, dtype=torch.float32):
    sd = {k: v.detach().to(image.device, dtype) for k, v in sd.items()}
    g = lambda k: sd["base." + k]                                                # noqa: E731
    lin = lambda x, k, relu=True: (F.relu if relu else (lambda t: t))(F.linear(x, g(k + ".weight"), g(k + ".bias")))  # noqa: E731
    x = image.to(dtype)
    for i, pool in ((0, False), (2, True), (5, True), (8, True), (11, True)):
        x = F.relu(F.conv2d(x, g(f"imgCNN.{i}.weight"), g(f"imgCNN.{i}.bias"), padding=1))
        if pool:
            x = F.max_pool2d(x, 2, 2)
    x = F.relu(F.conv2d(x, g("imgCNN.14.weight"), g("imgCNN.14.bias"), stride=2, padding=1))
    img = x.reshape(x.shape[0], -1)
    o = F.relu(F.conv2d(occupancy.to(dtype), g("occupancyCNNMLP.0.weight"), g("occupancyCNNMLP.0.bias"), stride=2, padding=1))
    o = F.relu(F.conv2d(o, g("occupancyCNNMLP.2.weight"), g("occupancyCNNMLP.2.bias"), stride=2, padding=1))
    o = lin(lin(o.reshape(o.shape[0], -1), "occupancyCNNMLP.5"), "occupancyCNNMLP.7")
    flat = lin(lin(img, "cnnMlp.0"), "cnnMlp.2")
    motor = lin(lin(image_feat.to(dtype), "motorMlp.0"), "motorMlp.2")
    im = lin(lin(flat + motor + o, "imgMotorMlp.0"), "imgMotorMlp.2")
    # one GRU step (torch.nn.GRU, gate order r, z, n) from rnn_hxs * masks
    h = rnn_hxs.to(dtype) * masks.to(dtype)
    gi = F.linear(im, g("gru.weight_ih_l0"), g("gru.bias_ih_l0"))
    gh = F.linear(h, g("gru.weight_hh_l0"), g("gru.bias_hh_l0"))
    ir, iz, inn = gi.chunk(3, 1)
    hr, hz, hn = gh.chunk(3, 1)
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    h1 = (1 - z) * torch.tanh(inn + r * hn) + z * h
    imr = lin(h1, "imgMotorMlp2.0")
    snd = lin(lin(lin(goal_sound_feat.to(dtype), "soundMlp.0"), "soundMlp.2"), "soundMlp.4")
    fusion = lin(lin(snd + flat, "fusionMlp.0"), "fusionMlp.2")
    x = lin(lin(fusion + imr, "mlp_all.0"), "mlp_all.2")
    value = lin(lin(lin(x, "critic.0"), "critic.2"), "critic_linear", relu=False)
    feats = lin(lin(x, "actor.0"), "actor.2")
    logits = F.linear(feats, sd["dist.linear.weight"], sd["dist.linear.bias"])
    return value, feats, logits, h1
