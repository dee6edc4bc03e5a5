"""The convolutional autoencoder that pre-trains the conv stem, with the reference's module layout.

`CAE(in_channels, h_channels)` == lib/models/convolutional_autoencoder.py: encoder
Conv2d(in, h, 3, padding 1) -> LeakyReLU -> MaxPool2d(2) — the stem of QNet, ActorCriticNet and
PolicyNetwork — and decoder ConvTranspose2d(h, in, kernel 2, stride 2, output_padding 1) ->
Sigmoid. state_dict keys `encoder.0.weight [32, 3, 3, 3]`, `encoder.0.bias`, `decoder.0.weight
[32, 3, 2, 2]`, `decoder.0.bias [3]`: checkpoints, and a saved `model.encoder`, interchange with
the reference's.

forward(x):
  f32 [n, 3, 15, 15]              plain torch (CPU or GPU);
  packed int32 [n, 22] on the GPU the HIP stem (csrc/mz_stem.hip) + mz_cae_decode
                                  (csrc/mz_cae.hip); inference only — training goes through
                                  mazerl.cae.cae_loss, which never writes Y to memory.
"""
import torch
import torch.nn as nn


class CAE(nn.Module):
    def __init__(self, in_channels=3, h_channels=32):
        super().__init__()
        self.encoder = nn.Sequential(
            nn.Conv2d(in_channels, h_channels, kernel_size=3, stride=1, padding=1),
            nn.LeakyReLU(),
            nn.MaxPool2d(2, 2),
        )
        self.decoder = nn.Sequential(
            nn.ConvTranspose2d(h_channels, in_channels, kernel_size=2, stride=2, output_padding=1),
            nn.Sigmoid(),
        )

    def forward(self, x):
        if x.dtype == torch.int32 and x.dim() == 2:
            return self._packed(x)
        return self.decoder(self.encoder(x))

    @torch.no_grad()
    def _packed(self, bits):
        from ... import _native as N
        from ...cae import stem_features_only
        feat = stem_features_only(bits, self.encoder[0])
        dec = self.decoder[0]
        if tuple(dec.weight.shape) != (32, 3, 2, 2):
            raise ValueError("the packed path implements ConvTranspose2d(32, 3, 2, stride 2)")
        n = bits.shape[0]
        out = torch.empty(n, 3, 15, 15, dtype=torch.float32, device=bits.device)
        if n == 0:
            return out
        N.check(N.load().mz_cae_decode(feat.data_ptr(), feat.shape[1], n,
                                       dec.weight.detach().contiguous().data_ptr(),
                                       dec.bias.detach().contiguous().data_ptr(), out.data_ptr(),
                                       torch.cuda.current_stream(bits.device).cuda_stream))
        return out
