"""Shapes shared by tests/test_global_rows_cpu.py and tests/test_gpu_global_rows.py: where `auto` changes the tile flavour.

The switch from 4-row to 16-row tiles depends on the hidden size (workgroups that co-reside on a CU, the measured cost ratio of
the two flavours), so it is found with the host query, never written down.  Batches are searched over the multiples of 32: the
tests cut them into eight equal shards."""
from stable_neural_sdes_amd import engine

KNOTS, STEPS, CHANNELS = 6, 5, 3          # L = 6 knots, five steps of dt = 1, C = 3
FOUR_ROW = ('lean', 'lean-streamed', 'mfma4')
SHARDS = 8


def elementwise_model(H):
    """The reference's neurallnsde field: embedded drift with time features, two-layer time-only noise MLP times y."""
    return engine.model_struct(CHANNELS, H, H, 2, 4, 17)


def net_model():
    """H = 64, latent-only drift, two-layer diffusion net (noise_option 18): the wave-pair kernels' configuration."""
    return engine.model_struct(CHANNELS, 64, 64, 2, 1, 18)


def path(model, batch, method='euler', **kw):
    return engine.forward_path(model, batch, KNOTS, STEPS, method, **kw)


def flip_batch(H, limit=1 << 16):
    """Smallest multiple of 32 rows at which `auto` leaves the 4-row tiles for the elementwise model (Euler)."""
    model = elementwise_model(H)
    assert path(model, 32) in FOUR_ROW
    for n in range(32, limit + 1, 32):
        if path(model, n) not in FOUR_ROW:
            return n
    raise AssertionError(f'H = {H}: auto stays on 4-row tiles up to {limit} rows')
