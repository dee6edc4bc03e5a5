"""REINFORCE: agents/rf_agent.py:10-129 under lib/trainers/value_based_trainer.py:25-92.

PolicyNetwork   same layers / names as the reference (`conv` stem + `fc` 1574 -> 1024 -> 512 -> 4:
                the Q-net's shapes, 2,140,548 parameters), so its state_dict loads. Packed int32
                windows [n, 22] go through the f32 HIP stem at the reference's 32 conv channels
                (as ActorCriticNet.forward); another width expands the bits and runs Conv2d.
select_action   softmax(logits / 2), one multinomial draw, log(p + 1e-10) of the draw and of all
                four entries (:73-86). The reference's test() samples too: there is no greedy mode.
get_returns     R = r + gamma R backwards over Python floats, float32, (R - mean) / (std + 1e-6)
                with the unbiased std (:88-99): NaN for a 1-step episode, zeros for constant
                returns.
reinforce_loss  optimize_model's loss (:101-118) as one torch expression over rows that carry
                their episode's baseline-subtracted return and length: per row
                f = (1/E)(-adv l_a - (coef / T)(-sum_k l_k exp(l_k))), l = log(softmax(x / tau) +
                1e-10). One whole episode with E = 1 is the reference's loss; E episodes give the
                mean of their losses. head_loss() is the same from one HIP launch
                (mz_rf_head_loss) on GPU tensors and this expression on CPU tensors.
cosine_lr       CosineAnnealingLR(T_max=200, eta_min=1e-5) in closed form (:68, :128); the
                reference steps it past T_max and the rate rises again.
RFAgent         single-env drop-in with the reference's constructor and methods.
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.optim as optim
from torch.optim import lr_scheduler

from .linear import GraphSafeLinear

WINDOW = (15, 15)
LOG_EPS = 1e-10
T_MAX, ETA_MIN = 200, 1e-5


def _expand_bits(bits, channels):
    """Packed windows int32 [n, 22] -> f32 [n, channels, 15, 15] (bit j of the row = element j)."""
    n_el = channels * WINDOW[0] * WINDOW[1]
    j = torch.arange(n_el, device=bits.device)
    w = (bits.to(torch.int64)[:, j // 32] >> (j % 32)) & 1
    return w.to(torch.float32).view(-1, channels, *WINDOW)


class PolicyNetwork(nn.Module):
    WINDOW_SIZE = WINDOW

    def __init__(self, in_channels=3, n_observations=6, n_actions=4, h_channels=32, hidden_dim=1024):
        super().__init__()
        self.in_channels = in_channels
        self.conv = nn.Sequential(nn.Conv2d(in_channels, h_channels, kernel_size=3, stride=1, padding=1),
                                  nn.LeakyReLU(), nn.MaxPool2d(2, 2))
        d0 = h_channels * (WINDOW[0] // 2) * (WINDOW[1] // 2) + n_observations
        self.fc = nn.Sequential(GraphSafeLinear(d0, hidden_dim), nn.LeakyReLU(),
                                GraphSafeLinear(hidden_dim, hidden_dim // 2), nn.LeakyReLU(),
                                GraphSafeLinear(hidden_dim // 2, n_actions))
        nn.init.xavier_uniform_(self.conv[0].weight)

    def forward(self, x):
        s, w = x
        if w.dtype == torch.int32 and w.dim() == 2:  # packed windows
            conv = self.conv[0]
            if w.is_cuda and tuple(conv.weight.shape) == (32, 3, 3, 3):
                from .stem import stem_features  # the HIP f32 stem (Conv -> LeakyReLU -> MaxPool)
                return self.fc(stem_features(w, s, conv, 0.0, None, 0))
            w = _expand_bits(w, self.in_channels)
        fw = self.conv(w)
        return self.fc(torch.cat((fw.view(fw.shape[0], -1), s), dim=1))


def select_action(net, state, temperature=2.0):
    """(action [n, 1], log-prob of the draw [n], log(p + 1e-10) [n, 4]) for a batch of states."""
    logits = net(state)
    probs = F.softmax(logits / temperature, dim=-1)
    action = torch.multinomial(probs, num_samples=1)
    logp = torch.log(probs + LOG_EPS)
    return action, torch.log(probs.gather(1, action).squeeze(1) + LOG_EPS), logp


def get_returns(rewards, gamma, device=None):
    acc, out = 0, []
    for r in reversed(list(rewards)):
        acc = r + gamma * acc
        out.append(acc)
    out.reverse()
    ret = torch.tensor(out, dtype=torch.float32, device=device)
    return (ret - ret.mean()) / (ret.std() + 1e-6)


def reinforce_loss(logits, action, adv, length=None, episodes=1, temperature=2.0,
                   entropy_coef=0.01):
    """`adv`: each row's return minus its episode's mean return (optimize_model's baseline);
    `length`: each row's episode length (None: the rows are one whole episode); `episodes`: the
    number of episodes the rows come from (a number or a tensor)."""
    n = logits.shape[0]
    logp = torch.log(F.softmax(logits / temperature, dim=-1) + LOG_EPS)
    la = logp.gather(1, action.reshape(n, 1).long()).squeeze(1)
    ent = -(logp * logp.exp()).sum(dim=1)
    T = float(n) if length is None else length.to(logp.dtype)
    total = (-la * adv.detach()).sum() - entropy_coef * (ent / T).sum()
    return total / episodes


class _RFHeadLoss(torch.autograd.Function):
    """reinforce_loss and its gradient w.r.t. the logits from one HIP launch (mz_rf_head_loss:
    float64 row arithmetic, the chunk's loss summed in a fixed order) instead of ~20 small torch
    kernels forward and backward. `episodes`: int32 device scalar (the pooled-episode count)."""

    @staticmethod
    def forward(ctx, logits, action, adv, length, episodes, temperature, entropy_coef):
        from .. import _native as N
        b, dev = logits.shape[0], logits.device
        if logits.shape[1] != 4 or logits.dtype != torch.float32:
            raise ValueError("mz_rf_head_loss takes f32 rows of 4 logits")
        logits = logits.contiguous()
        action = action.reshape(-1).contiguous().long()
        adv = adv.reshape(-1).contiguous().float()
        length = length.reshape(-1).contiguous().to(torch.int32)
        if action.numel() != b or adv.numel() != b or length.numel() != b:
            raise ValueError("one action, advantage and episode length per logits row")
        if episodes.dtype != torch.int32 or episodes.numel() != 1 or episodes.device != dev:
            raise ValueError("episodes: an int32 scalar on the logits' device")
        loss = torch.zeros(1, dtype=torch.float32, device=dev)
        dlogits = torch.empty(b, 4, dtype=torch.float32, device=dev)
        N.check(N.load().mz_rf_head_loss(
            logits.data_ptr(), logits.stride(0) if b else 4, action.data_ptr(), adv.data_ptr(),
            length.data_ptr(), episodes.data_ptr(), b, float(temperature), float(entropy_coef),
            loss.data_ptr(), dlogits.data_ptr(), 4, torch.cuda.current_stream(dev).cuda_stream))
        ctx.save_for_backward(dlogits)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g, None, None, None, None, None, None


def head_loss(logits, action, adv, length, episodes, temperature=2.0, entropy_coef=0.01):
    """reinforce_loss over pool rows: the HIP launch on GPU tensors, the torch expression on CPU
    tensors."""
    if logits.is_cuda:
        return _RFHeadLoss.apply(logits, action, adv, length, episodes, temperature, entropy_coef)
    return reinforce_loss(logits, action, adv, length, episodes, temperature, entropy_coef)


def cosine_lr(k, lr, t_max=T_MAX, eta_min=ETA_MIN):
    """The learning rate after k scheduler steps."""
    return eta_min + (lr - eta_min) * (1.0 + math.cos(math.pi * k / t_max)) / 2.0


class RFAgent:
    def __init__(self, env, lr, gamma, device):
        self.lr, self.gamma = lr, gamma
        self.env, self.device = env, device
        obs, _ = env.reset()
        n_obs = len(np.concatenate([obs[k] for k in obs if k != "window"]))
        self.policy_net = PolicyNetwork(3, n_obs, env.action_space.n, 32).to(device)
        self.policy_net.train()
        self.optimizer = optim.AdamW(self.policy_net.parameters(), lr)
        self.lr_scheduler = lr_scheduler.CosineAnnealingLR(self.optimizer, T_max=T_MAX, eta_min=ETA_MIN)

    def get_probs(self, state):
        return self.policy_net(state)

    def select_action(self, state, temperature=2):
        state = (state[0].to(self.device), state[1].to(self.device))
        action, lp, logp = select_action(self.policy_net, state, temperature)
        return action.item(), lp[0], logp

    def get_returns(self, rs):
        return get_returns(rs, self.gamma, self.device)

    def optimize_model(self, action_probabilities, probabilities, returns):
        lp = torch.stack(action_probabilities).to(self.device)
        logp = torch.stack(probabilities).to(self.device)
        returns = returns.to(self.device)
        adv = (returns - returns.mean()).detach()
        entropy = -(logp * logp.exp()).sum(dim=1).mean()
        loss = (-lp * adv).sum() - 0.01 * entropy
        self.optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.policy_net.parameters(), 1.0)
        self.optimizer.step()

    def scheduler_step(self):
        self.lr_scheduler.step()
