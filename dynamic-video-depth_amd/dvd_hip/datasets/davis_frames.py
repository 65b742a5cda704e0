"""`--dataset davis_frames`: the video of `--dataset davis_sequence`, trained from its frame and flow-pair files through a
device-resident store (datasets/frame_store.py) instead of from `.pt` pair packs.  Same flags plus `--store_gb`; the object
is not indexed like a map-style dataset: its `loader()` is the training view (pass it to `train_epoch` as the loader and as
`reset_dataset`), its `frames()` the validation / test view."""
import torch

from . import davis_sequence
from .frame_store import Catalogue, FrameStore


class Dataset(object):
    @classmethod
    def add_arguments(cls, parser):
        parser, unique = davis_sequence.Dataset.add_arguments(parser)
        parser.add_argument('--store_gb', type=float, default=64.0,
                            help='HBM the frame store may take; a video that needs more is an error before anything is allocated')
        return parser, unique

    def __init__(self, opt, mode='train', model=None, data_root=None, device=None, store=None):
        assert mode in ('train', 'vali')
        self.opt, self.mode = opt, mode
        if getattr(opt, 'subsample', False):
            raise ValueError('--dataset davis_frames has no --subsample mode')
        if store is None:                    # (the train and the vali object of a run share one: pass store=train.store)
            root = data_root or getattr(opt, 'data_root', None) or davis_sequence.DATA_ROOT
            cat = Catalogue(root, opt.track_id, opt.gaps, manual_seed=getattr(opt, 'manual_seed', None))
            device = device if device is not None else torch.device('cuda', torch.cuda.current_device())
            store = FrameStore(cat, device, budget_gb=getattr(opt, 'store_gb', 64.0))
        self.store = store

    def loader(self, group_gaps=False, rank=0, world=1):
        n = int(getattr(self.opt, 'pairs_per_step', 0) or 0)
        if n <= 0:
            raise ValueError('--dataset davis_frames needs --pairs_per_step N > 0')
        return self.store.loader(n, group_gaps=group_gaps, rank=rank, world=world, repeat=getattr(self.opt, 'repeat', 1))

    def frames(self, batch_size=1):
        return self.store.frames(batch_size)
