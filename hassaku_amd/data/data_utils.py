"""`get_dataloader` factory and the dataset registry (data/data_utils.py:36-47,317-375).

The reference's download / k-core / split preprocessing needs the network and is out of scope; processed
datasets in the 5-CSV layout (or hassaku_amd.data.synthetic) are consumed as they are.  `ml100k` is
added to the registry: BASELINE.json names it and the reference ships a processor but no enum member.
"""
import enum
import logging
import os

import numpy as np
import pandas as pd
import torch
from scipy import sparse as sp
from torch.utils.data import DataLoader

from hassaku_amd.data.dataloader import NegativeSampler, TrainDataLoader
from hassaku_amd.data.dataset import ECFTrainRecDataset, FullEvalDataset, TrainRecDataset


class DatasetsEnum(enum.Enum):
    ml1m = enum.auto()
    ml10m = enum.auto()
    amazonvid2018 = enum.auto()
    lfm2b2020 = enum.auto()
    deliveryherosg = enum.auto()
    lfm2bdemobias = enum.auto()
    deezer = enum.auto()
    ml100k = enum.auto()


class _EvalLoader:
    """Evaluation 'loader' for the HIP evaluator: carries the dataset and the batch size; iterating it yields
    the reference's dense (u, arange(I), labels) batches for generic algorithms."""

    def __init__(self, dataset: FullEvalDataset, batch_size: int, num_workers: int = 0):
        self.dataset, self.batch_size, self.num_workers = dataset, batch_size, num_workers

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        return iter(DataLoader(self.dataset, batch_size=self.batch_size, num_workers=0))


def get_dataloader(conf: dict, split_set: str):
    running = conf['running_settings']
    if split_set == 'train':
        # ECF's train dataset also carries the item x tag matrix (data/data_utils.py:325-328)
        train_dataset_class = ECFTrainRecDataset if conf.get('alg') == 'ecf' else TrainRecDataset
        dataset = train_dataset_class(data_path=conf['dataset_path'])
        sampler = NegativeSampler(train_dataset=dataset, n_neg=conf['neg_train'],
                                  neg_sampling_strategy=conf['train_neg_strategy'])
        loader = TrainDataLoader(sampler, dataset, batch_size=conf['train_batch_size'], shuffle=True,
                                 num_workers=running.get('train_n_workers', 0), device=conf.get('device', 'cuda'))
        logging.info('Built Train DataLoader batch_size=%d', conf['train_batch_size'])
        return loader
    if split_set in ('val', 'test'):
        loader = _EvalLoader(FullEvalDataset(data_path=conf['dataset_path'], split_set=split_set),
                             batch_size=conf['eval_batch_size'], num_workers=running.get('eval_n_workers', 0))
        logging.info('Built %s DataLoader batch_size=%d', split_set, conf['eval_batch_size'])
        return loader
    raise ValueError(f"split_set value '{split_set}' is invalid! Please choose from [train, val, test]")


# ------------------------------------------------------------------------------------------------
# the two pairs of matrices of the calibration metrics (data/data_utils.py:378-498): user x bin and item x bin
# distributions over the train split.  Built once per evaluation on the host with the numpy / scipy calls of the
# reference, in float32 as there, so the results are the reference's bit for bit.
# ------------------------------------------------------------------------------------------------
def _calibration_inputs(path_to_dataset_folder: str):
    """(n_users, n_items, train user ids, train item ids, the processed_dataset directory)"""
    folder = os.path.join(path_to_dataset_folder, 'processed_dataset')
    n_users = len(pd.read_csv(os.path.join(folder, 'user_idxs.csv')))
    n_items = len(pd.read_csv(os.path.join(folder, 'item_idxs.csv')))
    train = pd.read_csv(os.path.join(folder, 'listening_history_train.csv'))[['user_idx', 'item_idx']]
    return n_users, n_items, train.user_idx.to_numpy(), train.item_idx.to_numpy(), folder


def build_user_and_item_tag_matrix(path_to_dataset_folder: str, alpha_smoothening: float = .01):
    """-> (user_tag_mtx [n_users, n_tags], item_tag_mtx [n_items, n_tags]), float32 torch tensors.

    Item rows: 1 / (number of the item's tags) on its tags (tag_idxs.csv, item_tag_idxs.csv), so an item with several
    tags splits its weight among them (Steck, Calibrated Recommendations, RecSys 2018); an untagged item is a zero row.
    User rows: the mean of the rows of the user's train items (an interaction listed n times counts n times), smoothed
    with alpha / n_tags (Eq. 7 there).  A user without train items keeps the NaN row 0 / 0 gives."""
    assert 0 <= alpha_smoothening <= 1, 'Alpha value out of bounds'
    n_users, n_items, users, items, folder = _calibration_inputs(path_to_dataset_folder)
    n_tags = len(pd.read_csv(os.path.join(folder, 'tag_idxs.csv')))
    item_tags = pd.read_csv(os.path.join(folder, 'item_tag_idxs.csv'))
    item_mtx = np.zeros((n_items, n_tags), dtype=np.float32)
    item_mtx[item_tags.item_idx.to_numpy(), item_tags.tag_idx.to_numpy()] = 1.
    with np.errstate(invalid='ignore'):
        item_mtx /= item_mtx.sum(-1)[:, None]
    item_mtx[np.isnan(item_mtx)] = 0.
    train = sp.csr_matrix((np.ones(len(users), dtype=np.int16), (users, items)), shape=(n_users, n_items))
    user_mtx = train @ item_mtx
    with np.errstate(invalid='ignore', divide='ignore'):
        user_mtx /= np.asarray(train.sum(-1))
    user_mtx = alpha_smoothening / n_tags + (1 - alpha_smoothening) * user_mtx
    return torch.tensor(user_mtx), torch.from_numpy(item_mtx)


POP_BUCKET_ENDS = (.2, .8)   # cumulative share of the interactions at which the head and the middle bucket end


def build_user_and_item_pop_matrix(path_to_dataset_folder: str, alpha_smoothening: float = .01):
    """-> (user_pop_mtx [n_users, 3], item_pop_mtx [n_items, 3]), float32 torch tensors.

    Items in order of falling train popularity (np.argsort of the negated shares, ties as that call leaves them) go to
    bucket 0 while the cumulative share, the item's own included, stays below .2, to bucket 1 while below .8, else to
    bucket 2; an item row is one-hot.  User rows: bucket counts of the user's train items divided by their own sum,
    smoothed with alpha / 3.  A user without train items keeps the NaN row."""
    assert 0 <= alpha_smoothening <= 1, 'Alpha value out of bounds'
    n_users, n_items, users, items, _ = _calibration_inputs(path_to_dataset_folder)
    train = sp.csr_matrix((np.ones(len(users), dtype=np.float32), (users, items)), shape=(n_users, n_items))
    share = np.asarray(train.sum(0)).ravel()
    share /= share.sum()
    order = np.argsort(-share)
    buckets = []
    mass = 0
    for item in order:
        mass += share[item]          # float32 running sum, as the thresholds were tuned on
        buckets.append(0 if mass < POP_BUCKET_ENDS[0] else 1 if mass < POP_BUCKET_ENDS[1] else 2)
    item_mtx = sp.csr_matrix((np.ones(n_items, dtype=np.float32), (order, buckets)), shape=(n_items, 3))
    user_mtx = (train @ item_mtx).toarray()
    with np.errstate(invalid='ignore'):
        user_mtx /= user_mtx.sum(-1)[:, None]
    user_mtx = alpha_smoothening / 3 + (1 - alpha_smoothening) * user_mtx
    return torch.tensor(user_mtx), torch.tensor(item_mtx.toarray())
