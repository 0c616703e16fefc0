"""The readout heads of the wrappers and the shapes tests/test_gpu_wrappers.py holds snsde_readout_head to float64 at (moved here
unchanged so that other tests can share them).  Plain data, importable without a GPU."""
import torch

HEAD_KINDS = ['classification', 'forecasting', 'ists', 'plain_bn']
# (leading dimensions of x, in_features, hidden, out_features): rows 3, 9 and 37 are ragged tiles, hidden 300 and 512 take two
# output features per thread, in_features 40 and 200 are no multiple of the kernel's 32-column slab
HEAD_SHAPES = [((1024,), 128, 128, 1), ((37,), 64, 64, 3), ((5, 10), 256, 256, 14), ((9,), 40, 72, 5),
               ((3,), 16, 300, 2), ((130,), 200, 512, 7), ((2050,), 128, 128, 20)]


def heads(H, Hh, O):
    nn = torch.nn
    return {
        'classification': nn.Sequential(nn.Linear(H, Hh), nn.BatchNorm1d(Hh), nn.ReLU(), nn.Dropout(0.1), nn.Linear(Hh, O)),
        'forecasting': nn.Sequential(nn.Linear(H, Hh), nn.ReLU(), nn.Linear(Hh, O)),
        'ists': nn.Sequential(nn.Tanh(), nn.Linear(H, Hh), nn.ReLU(), nn.Linear(Hh, O)),
        'plain_bn': nn.Sequential(nn.Linear(H, Hh), nn.BatchNorm1d(Hh, affine=False), nn.ReLU(), nn.Linear(Hh, O, bias=False)),
    }


def make_head(kind, shape, device):
    """(head in eval mode with drawn running statistics, the (input_tanh, linear1, batchnorm or None, linear2) the kernel takes)."""
    lead, H, Hh, O = shape
    torch.manual_seed(hash((kind, H, Hh)) % 1000)
    head = heads(H, Hh, O)[kind].to(device)
    for m in head:
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.normal_(); m.running_var.uniform_(0.3, 2.0)
            if m.weight is not None:
                m.weight.data.uniform_(0.5, 1.5); m.bias.data.normal_()
    head.eval()
    mods = [m for m in head if isinstance(m, (torch.nn.Linear, torch.nn.BatchNorm1d))]
    return head, (isinstance(head[0], torch.nn.Tanh), mods[0], mods[1] if len(mods) == 3 else None, mods[-1])   # the kernel itself: any size
