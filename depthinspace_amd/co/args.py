"""Command-line flags of the reference (/root/reference/co/args.py:30-73): same names and defaults."""
import argparse


def str2bool(v):
    """reference co/utils.py:32-40"""
    if isinstance(v, bool):
        return v
    if v.lower() in ('yes', 'true', 't', 'y', '1'):
        return True
    if v.lower() in ('no', 'false', 'f', 'n', '0'):
        return False
    raise argparse.ArgumentTypeError('Boolean value expected.')


PSEUDO_GT_SOURCES = ('multi_frame', 'raycast_gt', 'raycast_sgm', 'raycast_single_frame', 'raycast_multi_frame')


def pseudo_gt_stem(source):
    """the file stem a --pseudo_gt_source names: multi_frame -> multi_frame_disp, raycast_X -> raycast_X"""
    if source not in PSEUDO_GT_SOURCES:
        raise ValueError(f'pseudo_gt_source is one of {PSEUDO_GT_SOURCES}, not {source!r}')
    return 'multi_frame_disp' if source == 'multi_frame' else source


def get_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--data_type', default='synthetic', choices=['synthetic', 'real'], type=str)
    parser.add_argument('--cmd', help='Start training or test', default='resume',
                        choices=['retrain', 'resume', 'retest', 'test_init'], type=str)
    parser.add_argument('--epoch', help='If larger than -1, retest on the specified epoch', default=-1, type=int)
    parser.add_argument('--epochs', help='Training epochs', default=100, type=int)
    parser.add_argument('--warmup_epochs', default=150, type=int,
                        help='Number of epochs where SGM Disparities are used as supervisor on the real dataset')
    parser.add_argument('--lcn_radius', help='Radius of the window for LCN pre-processing', default=5, type=int)
    parser.add_argument('--max_disp', help='Maximum disparity', default=128, type=int)
    parser.add_argument('--track_length', help='Track length for geometric loss', default=4, type=int)
    parser.add_argument('--train_batch_size', help='Train Batch Size', default=8, type=int)
    parser.add_argument('--architecture', help='The architecture which will be used', default='single_frame',
                        choices=['single_frame', 'multi_frame'], type=str)
    parser.add_argument('--use_pseudo_gt', help='Only applicable in single-frame model', default=False, type=str2bool)
    # (not in the reference) which fused disparity the pseudo-GT term reads: multi_frame -> <track>/multi_frame_disp.npz (DIS-MF's
    # output, the reference's), raycast_X -> <track>/raycast_X.npz (data/raycast.py --disp X), key `disp` in both.  A raycast map
    # has holes (0): any value but the default pair (multi_frame, 0) selects the masked term, ops.masked_l1_multi
    parser.add_argument('--pseudo_gt_source', help='Which fused disparity --use_pseudo_gt trains on (not in the reference)',
                        default='multi_frame', choices=list(PSEUDO_GT_SOURCES), type=str)
    parser.add_argument('--pseudo_gt_erode', help='Also leave out pixels within this many pixels of a hole of the pseudo ground '
                        'truth (not in the reference)', default=0, choices=[0, 1, 2, 3], type=int)
    # (not in the reference) backward of the geometric loss: float atomics, or order-free sums that repeat bit for bit
    parser.add_argument('--geo_bwd', help='Backward of the geometric loss; default: the DIS_GEO_BWD environment variable, else atomic',
                        default=None, choices=['atomic', 'det'], type=str)
    # (not in the reference) the optimiser: the reference hard-codes Adam(lr=1e-4) and passes no scheduler (train_val.py:55-58)
    parser.add_argument('--lr', help='Learning rate (not in the reference)', default=1e-4, type=float)
    parser.add_argument('--lr_step', help='Multiply the learning rate by --lr_gamma every this many epochs; 0: constant '
                        '(not in the reference)', default=0, type=int)
    parser.add_argument('--lr_gamma', help='Factor of --lr_step (not in the reference)', default=0.5, type=float)
    parser.add_argument('--max_grad_norm', help='Clip the gradient to this global L2 norm; default: no clipping '
                        '(not in the reference)', default=None, type=float)
    parser.add_argument('--skip_nonfinite', help='Skip a step whose gradient norm is inf / NaN (not in the reference)',
                        default=False, type=str2bool)
    return parser


def parse_args(argv=None):
    args, _ = get_parser().parse_known_args(argv)
    return args
