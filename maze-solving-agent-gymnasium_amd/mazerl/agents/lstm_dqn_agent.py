"""Recurrent DQN for one env: agents/lstm_dqn_agent.py (an nn.LSTMCell(6, 32) + nn.Linear(32, 4)
Q-network over the flat obs6 vector, trained from whole episodes, lib/replay_memory.py:26-43).

DQN        same attribute names (`lstm_cell`, `fc`, `hidden_state`, `cell_state`), state_dict keys
           and `reset_hidden_state` as the reference, so its checkpoints load and forward() returns
           the same bits. `unroll()` also returns the q values of every step.
DQNAgent   the reference's constructor and method names. The reference leaves the agent unfinished
           (no trainer drives it; optimize_model zips a list of episodes as if they were
           transitions; get_action prints a shape and explores over randrange(2); the hidden state
           is resized to the batch and never restored), so the semantics are fixed here, the same
           six as the vectorised trainer (trainers/drqn_trainer.py):
  1. acting state: (h, c) is zero at the first step of every episode and advances once per
     get_action with the parameters of that moment;
  2. exploration: with probability eps a uniform action over `explore_actions` (default: the
     env's action_space.n; 2 reproduces the reference's leftover);
  3. eps = final + (start - final) exp(-steps_done / decay), steps_done += 1 per get_action,
     update_steps_done() halves it;
  4. memorize(done, state, action, reward, next_state) buffers the step; on `done` the episode is
     stored whole: x_0 .. x_n, a_0 .. a_{n-1}, r_0 .. r_{n-1} (float32) and terminated
     (next_state is None, as the reference's trainers pass a terminal state);
  5. optimize_model: `batch_size` episodes by random.sample; the source net unrolled from zero
     state over x_0 .. x_{n-1}, the target net over x_0 .. x_n; y_t = r_t + gamma max_a
     Q'_{t+1}[a] (r_t alone at a terminated episode's last step; a truncated one bootstraps from
     x_n); loss = mean over all steps of (Q_t[a_t] - y_t)^2, no gradient through y; the
     reference's clamp_(-1, 1) per element and AdamW;
  6. nothing happens until the memory holds `batch_size` episodes.
window_td_loss is the loss of the vectorised trainer's replay windows (its departures 7-9: fixed
windows of T steps, stored recurrent state, burn-in) for one env's code; DQNAgent itself keeps
training on whole episodes.
"""
import math
import random
from collections import deque

import numpy as np
import torch
import torch.nn as nn
import torch.optim as optim
from torch.optim import lr_scheduler

T_MAX, ETA_MIN = 30, 1e-6
HIDDEN = 32


def epsilon_at(steps_done, start, final, decay):
    return final + (start - final) * math.exp(-1.0 * steps_done / decay)


class DQN(nn.Module):
    def __init__(self, input_size, n_actions, hidden_size, device):
        super().__init__()
        self.device = device
        self.hidden_size = hidden_size
        self.lstm_cell = nn.LSTMCell(input_size, hidden_size, device=device)
        self.fc = nn.Linear(hidden_size, n_actions).to(device)
        self.hidden_state = None
        self.cell_state = None

    def reset_hidden_state(self, batch_size):
        self.hidden_state = torch.zeros(batch_size, self.hidden_size).to(self.device)
        self.cell_state = torch.zeros(batch_size, self.hidden_size).to(self.device)

    def forward(self, x):
        """x [batch, seq, input]: advances (hidden_state, cell_state) over the sequence and
        returns the q values of its last step."""
        for i in range(x.size(1)):
            self.hidden_state, self.cell_state = self.lstm_cell(
                x[:, i, :], (self.hidden_state, self.cell_state))
        return self.fc(self.hidden_state)

    def unroll(self, x):
        """x [batch, seq, input] from zero state -> q [batch, seq, actions]; the carried state is
        left alone."""
        h = torch.zeros(x.size(0), self.hidden_size, dtype=x.dtype, device=x.device)
        c = torch.zeros_like(h)
        out = []
        for i in range(x.size(1)):
            h, c = self.lstm_cell(x[:, i, :], (h, c))
            out.append(self.fc(h))
        return torch.stack(out, dim=1)

    def unroll_from(self, x, h, c):
        """unroll() from the state (h, c) [batch, hidden] -> (q [batch, seq, actions], h, c)."""
        out = []
        for i in range(x.size(1)):
            h, c = self.lstm_cell(x[:, i, :], (h, c))
            out.append(self.fc(h))
        return torch.stack(out, dim=1), h, c


def td_loss(source, target, episodes, gamma):
    """The episode-batch loss (semantics 5). episodes: (x [n + 1, 6], a [n] long, r [n], term)."""
    total, steps = 0.0, 0
    for x, a, r, term in episodes:
        n = a.shape[0]
        q = source.unroll(x[None, :n])[0]
        with torch.no_grad():
            y = r + gamma * target.unroll(x[None])[0, 1:].max(dim=1)[0]
            if term:
                y[n - 1] = r[n - 1]
        total = total + ((q.gather(1, a[:, None]).squeeze(1) - y) ** 2).sum()
        steps += n
    return total / steps


def window_td_loss(source, target, windows, gamma, weights=None):
    """The loss of a batch of replay windows (trainers/drqn_trainer.py, departure 9). A window is
    (x [k + m + 1, 6], a [m] long, r [m], h0 [32], c0 [32], k, term): the observations of steps
    b .. s + m, the actions and rewards of the m training steps s .. s + m - 1, the state both nets
    start from at step b, the k = s - b burn-in steps, and term = the last training step is the
    last step of a terminated episode (its y is r alone). Burn-in steps carry no loss term and no
    gradient flows into them or through the state that enters step s. loss = sum (Q_t[a_t] -
    y_t)^2 / sum m. weights (one per window; None: all 1) are the importance weights of prioritized
    replay (departure 12): loss = sum_e w_e sum_t (Q_t[a_t] - y_t)^2 / sum m."""
    total, steps = 0.0, 0
    for e, (x, a, r, h0, c0, k, term) in enumerate(windows):
        m = a.shape[0]
        h, c = h0[None], c0[None]
        with torch.no_grad():
            if k:
                _, h, c = source.unroll_from(x[None, :k], h, c)
            y = r + gamma * target.unroll_from(x[None], h0[None], c0[None])[0][0, k + 1:].max(dim=1)[0]
            if term:
                y[m - 1] = r[m - 1]
        q = source.unroll_from(x[None, k:k + m], h, c)[0][0]
        sq = ((q.gather(1, a[:, None]).squeeze(1) - y) ** 2).sum()
        total = total + (sq if weights is None else weights[e] * sq)
        steps += m
    return total / steps


class DQNAgent:
    def __init__(self, env, learning_rate, starting_epsilon, final_epsilon, epsilon_decay,
                 discount_factor, batch_size, memory_size, target_update_frequency, device,
                 explore_actions=None):
        self.env, self.device = env, device
        self.learning_rate = learning_rate
        self.starting_epsilon, self.final_epsilon = starting_epsilon, final_epsilon
        self.epsilon_decay = epsilon_decay
        self.discount_factor = discount_factor
        self.batch_size = batch_size
        self.target_update_frequency = target_update_frequency
        obs, _ = env.reset()
        n_obs = len(np.concatenate([obs[k] for k in obs.keys()], axis=0))
        n_actions = env.action_space.n
        self.explore_actions = int(explore_actions or n_actions)
        self.source_net = DQN(n_obs, n_actions, HIDDEN, device).to(device)
        self.target_net = DQN(n_obs, n_actions, HIDDEN, device).to(device)
        self.source_net.reset_hidden_state(1)
        self.target_net.reset_hidden_state(1)
        self.memory = deque([], maxlen=memory_size)  # whole episodes
        self.buffer = []
        self.optimizer = optim.AdamW(self.source_net.parameters(), learning_rate)
        self.lr_scheduler = lr_scheduler.CosineAnnealingLR(self.optimizer, T_max=T_MAX,
                                                           eta_min=ETA_MIN)
        self.steps_done = 0
        self._fresh = True  # the next get_action starts an episode

    def epsilon(self):
        return epsilon_at(self.steps_done, self.starting_epsilon, self.final_epsilon,
                          self.epsilon_decay)

    def get_action(self, state):
        sample = random.random()
        eps = self.epsilon()
        self.steps_done += 1
        if self._fresh:
            self.source_net.reset_hidden_state(1)
            self._fresh = False
        with torch.no_grad():  # the state advances whether or not the step explores
            x = torch.as_tensor(state, dtype=torch.float32, device=self.device).reshape(1, 1, -1)
            q = self.source_net(x)
        if sample < eps:
            a = random.randrange(self.explore_actions)
            return torch.tensor([[a]], device=self.device, dtype=torch.long)
        return q.max(1)[1].view(1, 1)

    def memorize(self, done, state, action, reward, next_state):
        self.buffer.append((state, action, reward, next_state))
        if not done:
            return
        steps, self.buffer = self.buffer, []
        self._fresh = True
        f32 = lambda s: torch.as_tensor(s, dtype=torch.float32).reshape(-1).cpu()  # noqa: E731
        last = steps[-1][3]
        xs = [f32(s[0]) for s in steps]
        xs.append(torch.zeros_like(xs[0]) if last is None else f32(last))
        a = torch.tensor([int(s[1]) for s in steps], dtype=torch.long)
        r = torch.tensor([float(s[2]) for s in steps], dtype=torch.float32)
        self.memory.append((torch.stack(xs), a, r, last is None))

    def optimize_model(self):
        if len(self.memory) < self.batch_size:
            return None
        batch = [(x.to(self.device), a.to(self.device), r.to(self.device), term)
                 for x, a, r, term in random.sample(self.memory, self.batch_size)]
        loss = td_loss(self.source_net, self.target_net, batch, self.discount_factor)
        self.optimizer.zero_grad()
        loss.backward()
        for p in self.source_net.parameters():
            p.grad.data.clamp_(-1, 1)
        self.optimizer.step()
        return loss.item()

    def scheduler_step(self):
        self.lr_scheduler.step()

    def has_to_update(self, episode):
        return episode % self.target_update_frequency == 0

    def update_target(self):
        self.target_net.load_state_dict(self.source_net.state_dict())

    def update_steps_done(self):
        self.steps_done = self.steps_done // 2
