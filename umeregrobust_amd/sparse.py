"""A minimal stand-in for MinkowskiEngine's `SparseTensor`, as far as the reference's evaluation loop uses it
(evaluate.py:178-179, :190-192): built from features and `sparse_collate` coordinates, read back through `.F`, `.C` and
`.decomposed_features`.

Coordinates are int32 [N, 4] rows (batch index, x, y, z).  Rows keep the order they were given in: the feature network
(`umeregrobust_amd.models.ResUNetSmall2`) returns its output rows in input order, so `decomposed_features` splits by
batch index and keeps each cloud's rows in the order the collate produced them (MinkowskiEngine 0.5.4's behaviour on
unique input coordinates; parity unpinned)."""
import torch


class SparseTensor:
    def __init__(self, features, coordinates=None, device=None):
        if coordinates is None:
            raise TypeError("SparseTensor needs coordinates (int32 [N, 4]: batch index, x, y, z)")
        dev = torch.device(device) if device is not None else features.device
        coordinates = torch.as_tensor(coordinates)
        if coordinates.is_floating_point():
            coordinates = torch.floor(coordinates)
        self._C = coordinates.to(device=dev, dtype=torch.int32).contiguous()
        self._F = torch.as_tensor(features).to(dev)
        if self._C.dim() != 2 or self._C.shape[1] != 4:
            raise ValueError(f"coordinates must be [N, 4] (batch index, x, y, z), got {tuple(self._C.shape)}")
        if self._F.dim() != 2 or self._F.shape[0] != self._C.shape[0]:
            raise ValueError(f"features must be [N, C] with N = {self._C.shape[0]}, got {tuple(self._F.shape)}")
        self._batch_size = None

    @property
    def F(self):
        return self._F

    @property
    def C(self):
        return self._C

    features = F
    coordinates = C

    @property
    def device(self):
        return self._F.device

    @property
    def batch_size(self):
        """1 + the largest batch index (one device read, cached)."""
        if self._batch_size is None:
            self._batch_size = int(self._C[:, 0].max()) + 1 if self._C.shape[0] else 0
        return self._batch_size

    def _split(self, t):
        b = self._C[:, 0]
        return [t[b == i] for i in range(self.batch_size)]

    @property
    def decomposed_features(self):
        """[F of batch item 0, F of item 1, ...], each in row order."""
        return self._split(self._F)

    @property
    def decomposed_coordinates(self):
        return self._split(self._C[:, 1:])

    def __repr__(self):
        return f"SparseTensor(N={self._C.shape[0]}, channels={self._F.shape[1]}, device={self.device})"
