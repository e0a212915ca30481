#!/usr/bin/env python3
"""Command line of the MI355X path.  Same flags, defaults and run types as the reference's driver script
(run_experiment.py:8-36 there), so existing invocations keep working:

    python run_experiment.py -a mf -d ml1m -c conf.yml [-t train_val|test|train_val_test] [--log LEVEL]
                             [--measure_calibration]

Launched under `python -m torch.distributed.run --nproc-per-node N ...` it trains with one process per GPU
(hassaku_amd/dist.py); nothing else changes on the command line.
"""
import argparse
import logging
import sys

from hassaku_amd import experiment_helper as helper
from hassaku_amd.algorithms.algorithms_utils import (AVAILABLE_ALGORITHM_NAMES, OFFERED_ALGORITHM_NAMES,
                                                        algorithm_by_name)
from hassaku_amd.conf.conf_parser import parse_conf_file
from hassaku_amd.data.data_utils import DatasetsEnum

RUN_TYPES = {                      # -t value -> what it runs
    'train_val': helper.run_train_val,
    'test': helper.run_test,
    'train_val_test': helper.run_train_val_test,
}


def _flags():
    """(names, argparse keywords) for every flag of the reference's CLI."""
    later = ', '.join(n for n in AVAILABLE_ALGORITHM_NAMES if n not in OFFERED_ALGORITHM_NAMES)
    yield ('-a', '--algorithm'), dict(choices=sorted(AVAILABLE_ALGORITHM_NAMES), metavar='ALG',
                                      help=f"registry name of the model ({', '.join(sorted(OFFERED_ALGORITHM_NAMES))})"
                                           f' or {later}')
    yield ('-d', '--dataset'), dict(choices=sorted(m.name for m in DatasetsEnum), default='ml1m', metavar='DATASET',
                                    help='registry name of the dataset, default %(default)s')
    yield ('-c', '--conf_path'), dict(metavar='FILE', help='YAML (or JSON) file with the experiment configuration')
    yield ('-t', '--run_type'), dict(choices=sorted(RUN_TYPES), default='train_val_test',
                                     help='which phases to run, default %(default)s')
    yield ('--log',), dict(default='WARNING', metavar='LEVEL', help='logging level, default %(default)s')


def main(argv=None) -> int:
    cli = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    for names, kw in _flags():
        cli.add_argument(*names, type=str, **kw)
    # the reference's test driver has this as -c / --measure_calibration; -c is the conf path here
    cli.add_argument('--measure_calibration', action='store_true', default=False,
                     help='also report tag and popularity calibration metrics on the test split (sets the conf key '
                          'measure_calibration; needs tag_idxs.csv and item_tag_idxs.csv in the dataset)')
    opts = cli.parse_args(argv)
    logging.basicConfig(level=opts.log)
    conf = opts.conf_path
    if opts.measure_calibration:
        conf = parse_conf_file(conf)
        conf['measure_calibration'] = True
    RUN_TYPES[opts.run_type](algorithm_by_name(opts.algorithm), DatasetsEnum[opts.dataset], conf)
    return 0


if __name__ == '__main__':
    sys.exit(main())
