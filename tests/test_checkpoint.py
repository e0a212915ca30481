"""model.pth / conf.yml round trip with the reference: the on-disk formats on the output side of
the path (algorithms/base_classes.py:156-165, conf/conf_parser.py:46-51 of the reference).

tests/golden/g7_checkpoint/ is a run directory exactly as the reference leaves it (written by its own
save_model_to_path / save_yaml in oracle/gen_golden.py::gen_g7) plus the logits of the reloaded reference model."""
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN as GOLDEN_DIR

CKPT = os.path.join(GOLDEN_DIR, 'g7_checkpoint')


def _expected():
    with np.load(os.path.join(CKPT, 'expected.npz')) as z:
        return {k: z[k] for k in z.files}


def _conf():
    from hassaku_amd.conf.conf_parser import parse_conf_file
    return parse_conf_file(os.path.join(CKPT, 'conf.yml'))


def test_reference_conf_yml_parses_and_is_a_fixed_point_of_parse_conf():
    from hassaku_amd.algorithms.algorithms_utils import AlgorithmsEnum
    from hassaku_amd.conf.conf_parser import parse_conf
    from hassaku_amd.data.data_utils import DatasetsEnum
    conf = _conf()
    assert conf['alg'] == 'mf' and conf['dataset'] == 'ml1m' and conf['embedding_dim'] == 24
    assert conf['running_settings']['seed'] == 64 and conf['wd'] == 4e-5
    before = {k: (dict(v) if isinstance(v, dict) else v) for k, v in conf.items()}
    conf['device'] = 'cuda'                    # the only key a user must change: there is no CPU trainer here
    after = parse_conf(conf, AlgorithmsEnum[conf['alg']], DatasetsEnum[conf['dataset']])
    for k, v in before.items():                # every default the reference filled in is accepted unchanged
        if k not in ('device', 'time_run', 'model_path'):
            assert after[k] == v, k


def test_reference_model_pth_has_the_keys_and_shapes_of_our_state_dict():
    from hassaku_amd.algorithms.sgd_alg import SGDMatrixFactorization
    conf = _conf()
    sd = torch.load(os.path.join(CKPT, 'model.pth'), map_location='cpu')
    ours = SGDMatrixFactorization.build_from_conf(conf, types.SimpleNamespace(n_users=37, n_items=53)).state_dict()
    assert list(sd.keys()) == list(ours.keys())
    for k in sd:
        assert sd[k].shape == ours[k].shape and sd[k].dtype == ours[k].dtype, k
    ex = _expected()
    for k in sd:
        assert np.array_equal(sd[k].numpy(), ex['sd.' + k]), k


@pytest.mark.gpu
def test_reference_checkpoint_loads_and_scores_like_the_reference():
    from hassaku_amd.algorithms.sgd_alg import SGDMatrixFactorization
    conf, ex = _conf(), _expected()
    model = SGDMatrixFactorization.build_from_conf(conf, types.SimpleNamespace(n_users=37, n_items=53)).to('cuda')
    model.load_model_from_path(CKPT)
    for k, v in model.state_dict().items():
        assert np.array_equal(v.cpu().numpy(), ex['sd.' + k]), k
    out = model.predict(torch.from_numpy(ex['u_idx']).cuda(), torch.from_numpy(ex['i_idx']).cuda()).cpu().numpy()
    assert np.abs(out - ex['logits']).max() <= 1e-5 * np.abs(ex['logits']).max()


def test_our_checkpoint_loads_in_the_reference(tmp_path):
    """The other direction: a run directory written by this package is read back the way the reference reads one.

    The reference's readers are restated here, not imported: conf.yml goes through yaml.safe_load
    (conf/conf_parser.py:32-43 of the reference), model.pth through torch.load with its default arguments and a strict
    load_state_dict into the reference's model (algorithms/base_classes.py:161-165).  What that strict load needs --
    the reference model's state_dict keys, shapes and dtypes -- is pinned by the model.pth the reference itself wrote
    into tests/golden/g7_checkpoint/."""
    import yaml
    from hassaku_amd.algorithms.sgd_alg import SGDMatrixFactorization
    from hassaku_amd.conf.conf_parser import save_yaml
    conf = _conf()
    ds = types.SimpleNamespace(n_users=37, n_items=53)
    torch.manual_seed(5)
    ours = SGDMatrixFactorization.build_from_conf(conf, ds)
    with torch.no_grad():
        for p in ours.parameters():
            p.add_(torch.randn_like(p) * 0.2)
    ours.save_model_to_path(str(tmp_path))
    save_yaml(str(tmp_path), conf)
    with open(os.path.join(str(tmp_path), 'conf.yml')) as fh:
        ref_conf = yaml.safe_load(fh)
    assert ref_conf == conf
    with open(os.path.join(CKPT, 'conf.yml')) as fh:
        assert sorted(ref_conf) == sorted(yaml.safe_load(fh))   # every key the reference writes, no other
    ref_layout = torch.load(os.path.join(CKPT, 'model.pth'))    # the reference model's own state_dict
    sd = torch.load(os.path.join(str(tmp_path), 'model.pth'))
    assert isinstance(sd, dict) and list(sd.keys()) == list(ref_layout.keys())
    for k, v in ref_layout.items():
        assert torch.is_tensor(sd[k]) and sd[k].shape == v.shape and sd[k].dtype == v.dtype, k
        assert sd[k].device.type == 'cpu', k                   # the reference loads without map_location
    for k, v in ours.state_dict().items():
        assert torch.equal(sd[k], v), k
