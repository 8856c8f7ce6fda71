#!/usr/bin/env python
"""Fine-tune a HiFi-GAN or BigVGAN vocoder on the fine-tuning data set, on the GPU
    python scripts/train_vocoder.py -ft FINE_TUNING_DATASET -cfg CONFIG_JSON -g G_CKPT [-do DO_CKPT] -o OUT_DIR [--steps 1000]
                                    [--batch_size 16] [--segment_size 8192] [--compute_dtype fp32] [--checkpoint_interval 500]
                                    [--seed 1234] [--second_discriminator msd] [--mel_loss single]

  -ft    the `fine_tuning_dataset` directory `daft_exprt/fine_tune.py` writes: `<speaker>/<file>.npy` (teacher-forced mel) and
         `<speaker>/<file>.wav` (the cropped recording) per utterance
  -cfg   the `config.json` of the pretrained generator: HiFi-GAN's (V1 and V3 qualify: every stage a multiple of 32 channels) or, with
         an `activation` key, BigVGAN's (the 512-channel base models qualify, the 1536-channel models' 48- / 24-channel tail does not)
  -g     the pretrained generator checkpoint `g_XXXXXXXX`
  -do    the discriminator / optimiser checkpoint `do_XXXXXXXX` of THIS script to continue from; without it the discriminators
         start from their initialisation.  A file written with the other --second_discriminator is refused
  --second_discriminator  what trains beside the multi-period discriminator, for either generator family: `msd`, HiFi-GAN's multi-scale
         discriminator and recipe (lr 2e-4), or `mrd`, BigVGAN's multi-resolution discriminator (2-D convs over magnitude spectrograms at
         the config's `resolutions`, default [[1024, 120, 600], [2048, 240, 1200], [512, 50, 240]]) under BigVGAN's recipe: the config's
         `learning_rate` (default 1e-4) and `clip_grad_norm` (default 1000).  `do_%08d` then holds `mrd` in place of `msd`; that an
         upstream BigVGAN `do_` file loads has not been verified
  --mel_loss  the reconstruction term, independent of --second_discriminator: `single`, HiFi-GAN's L1 between two log-mels at the config's
         `n_fft`, weighted 45, or `multiscale`, BigVGAN-v2's sum over seven STFT resolutions of the L1 between log10-mels (window lengths
         `mel_loss_window_lengths`, default 32 ... 2048, with `mel_loss_n_mels`, default 5 ... 320, bands; weight `lambda_melloss`,
         default 15), one fused HIP kernel pair per resolution.  The scale list and the weight are restated from the papers and have not
         been checked against upstream's code
  -o     directory the checkpoints `g_%08d` / `do_%08d`, a copy of `config.json` and `vocoder_report.json` are written to;
         `scripts/synthesize.py -voc OUT_DIR/g_%08d` reads the result

The generator trains on the kernels it is run with (`daft_exprt/vocoder_train.py`); the discriminators and the losses are plain torch.
`vocoder_report.json` holds the utterances used / skipped / held out, per logged step the four loss terms and the held-out mel L1,
that L1 for the starting and the final generator, the generator's family and the steps per second.  The quality of a vocoder fine-tuned this way on real
speech has not been measured, and neither has the exchange of `do_` files with HiFi-GAN's own code."""
import argparse
import json
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'ubisoft-laforge-daft-exprt_amd')
sys.path.insert(0, PKG)

_logger = logging.getLogger('train_vocoder')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Fine-tune a HiFi-GAN vocoder on a fine-tuning data set')
    parser.add_argument('-ft', '--fine_tuning_dataset', required=True, help='directory of <speaker>/<file>.npy / .wav pairs')
    parser.add_argument('-cfg', '--config', required=True, help="HiFi-GAN's config.json")
    parser.add_argument('-g', '--generator', required=True, help='pretrained generator checkpoint g_XXXXXXXX')
    parser.add_argument('-do', '--discriminators', default=None, help='discriminator / optimiser checkpoint do_XXXXXXXX')
    parser.add_argument('-o', '--output_dir', required=True, help='directory for the checkpoints and the report')
    parser.add_argument('--steps', type=int, default=1000, help='training steps')
    parser.add_argument('--batch_size', type=int, default=16, help='segments per step')
    parser.add_argument('--segment_size', type=int, default=8192, help='samples per segment')
    parser.add_argument('--compute_dtype', default='fp32', choices=['fp32', 'bf16'], help="the generator's MFMA operand type")
    parser.add_argument('--checkpoint_interval', type=int, default=500, help='steps between checkpoints / validations')
    parser.add_argument('--seed', type=int, default=1234, help='seed of the segments and the discriminators')
    parser.add_argument('--second_discriminator', default='msd', choices=['msd', 'mrd'],
                        help="beside the MPD: HiFi-GAN's multi-scale (msd) or BigVGAN's multi-resolution (mrd) discriminator")
    parser.add_argument('--mel_loss', default='single', choices=['single', 'multiscale'],
                        help="the reconstruction term: HiFi-GAN's one log-mel (single) or BigVGAN-v2's seven resolutions (multiscale)")
    return parser.parse_args(argv)


def check_args(args):
    ''' the mistakes that can be told before the GPU is touched; SystemExit with one line '''
    if not os.path.isdir(args.fine_tuning_dataset):
        raise SystemExit(f'train_vocoder.py: no such fine-tuning data set: {args.fine_tuning_dataset}')
    for what, path in (('config', args.config), ('generator checkpoint', args.generator),
                       ('discriminator checkpoint', args.discriminators)):
        if path is not None and not os.path.isfile(path):
            raise SystemExit(f'train_vocoder.py: no such {what}: {path}')
    if min(args.steps, args.batch_size, args.segment_size, args.checkpoint_interval) < 1:
        raise SystemExit(f'train_vocoder.py: --steps {args.steps}, --batch_size {args.batch_size}, --segment_size {args.segment_size} '
                         f'and --checkpoint_interval {args.checkpoint_interval} must be at least 1')
    from daft_exprt import vocoder as V
    from daft_exprt.vocoder_train import LossMel, trainable_config
    try:
        config = V.load_config(args.config)
        V.validate_config(config)
        trainable_config(config)
        LossMel(config)
        if args.mel_loss == 'multiscale':
            from daft_exprt.mel_loss import MultiScaleMelLoss
            MultiScaleMelLoss(config).check_segment(args.segment_size)
    except (ValueError, json.JSONDecodeError) as e:
        raise SystemExit(f'train_vocoder.py: {args.config}: {e}')
    if args.segment_size % int(config['hop_size']):
        raise SystemExit(f'train_vocoder.py: --segment_size {args.segment_size} is not a multiple of the config\'s hop_size '
                         f'{config["hop_size"]}')
    return config


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(format='%(asctime)s [%(levelname)s] %(message)s', datefmt='%Y-%m-%d %H:%M:%S', level=logging.INFO)
    config = check_args(args)
    from daft_exprt.vocoder_train import fine_tune_vocoder
    os.makedirs(args.output_dir, exist_ok=True)
    try:
        report = fine_tune_vocoder(config, args.fine_tuning_dataset, args.generator, args.discriminators, out_dir=args.output_dir,
                                   steps=args.steps, batch_size=args.batch_size, segment_size=args.segment_size,
                                   compute_dtype=args.compute_dtype, checkpoint_interval=args.checkpoint_interval, seed=args.seed,
                                   second_discriminator=args.second_discriminator, mel_loss=args.mel_loss)
    except ValueError as e:                      # a mel of another hop / bin count, a short data set, a foreign checkpoint
        raise SystemExit(f'train_vocoder.py: {e}')
    path = os.path.join(args.output_dir, 'vocoder_report.json')
    with open(path, 'w', encoding='utf-8') as f:
        json.dump(report, f, indent=1)
    _logger.info(f'{report["steps"]} steps, held-out mel L1 {report["held_out_mel_l1_start"]} -> {report["held_out_mel_l1_final"]}, '
                 f'{report["steps_per_second"]} steps / s; {report.get("generator")} and the report written to {args.output_dir}')
    return report


if __name__ == '__main__':
    main()
