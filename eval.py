"""Prosody evaluation of converted speech (reference eval.py): pitch earth-mover's distance, word / phone F0-frame-error
and the length errors of every generated file under {base_path}/{method}/{trg}/ against {base_path}/orig/{trg}_{seq}.wav,
with the TextGrids of the Montreal Forced Aligner under the txtgrid/ folders.

    python eval.py --base_path results/vctk --method sr --target_speakers p231 p239

The F0 tracks (the reference runs amfm_decompy's YAAPT on the CPU, twice per file) come from dissc_amd.f0 in ragged
batches and are scored where they are by dissc_amd.metrics; every distinct original is tracked once, not once per source
speaker.  Same discovery and skip rules, same {method}_results.pkl and the same printed block as the reference.
The Whisper WER / CER leg is not part of this port: wer_* / cer_* stay 0 in the pickle and print as n/a.
"""
import argparse
import glob
import os
import pickle
from pathlib import Path

import numpy as np


def find_jobs(args):
    """the files reference eval.py:66-79 evaluates, in its order -> [(ref_wav, syn_wav, ref_grid, syn_grid | None)]"""
    orig = f'{args.base_path}/orig/'
    jobs = []
    for trg in args.target_speakers:
        print(f'--- speaker {trg} -----')
        for wav in glob.glob(f'{args.base_path}/{args.method}//{trg}/*.wav'):  # the reference's pattern: its file order
            name = wav.split('/')[-1]
            if trg in name:  # the target speaker's own utterance: a reconstruction, not a conversion
                continue
            seq = wav.split('_')[-1].split('.')[0]  # of the whole path, like the reference
            ref_wav = f'{orig}/{trg}_{seq}.wav'
            if not os.path.isfile(ref_wav):
                print('No reference recording: ', f'{trg}_{seq}.wav')
                continue
            stem = Path(wav).stem
            if stem.split('_')[0] == 'p270' and seq == '024':
                print('p270_024 is a problematic sample where content varies notably!')
                continue
            syn_grid = Path(wav).parent / f'txtgrid/{stem}.TextGrid'  # absent when MFA could not align the conversion
            jobs.append((ref_wav, wav, f'{orig}/txtgrid/{trg}_{seq}.TextGrid',
                         str(syn_grid) if os.path.isfile(syn_grid) else None))
    return jobs


def calc_errors(evaluator, args):
    """evaluator: dissc_amd.metrics.ProsodyEvaluator (anything with its ``evaluate(jobs)``)"""
    err_dict = {'wer_s': 0, 'wer_d': 0, 'cer_s': 0, 'cer_d': 0, 'len': [], 'emd': [], 'w_ffe': [], 'w_len': [],
                'p_ffe': [], 'p_len': []}
    for row in evaluator.evaluate(find_jobs(args)):
        for key in ('len', 'emd', 'p_len', 'p_ffe', 'w_len', 'w_ffe'):
            if key in row:
                err_dict[key].append(row[key])
    return err_dict


def log_results(err_dict, args, sr=16000):
    with open(f'{args.base_path}/{args.method}_results.pkl', 'wb') as f:
        pickle.dump(err_dict, f)

    print('WER: ', err_dict['wer_s'] / err_dict['wer_d'] if err_dict['wer_d'] else 'n/a')
    print('CER: ', err_dict['cer_s'] / err_dict['cer_d'] if err_dict['cer_d'] else 'n/a')
    print('EMD: ', np.mean(err_dict['emd']))
    print('Len Error: ', np.mean(err_dict['len']) / sr)

    print('Word Len Error: ', np.mean(err_dict['w_len']))
    print('Char Len Error: ', np.mean(err_dict['p_len']))
    print('Word FFE: ', np.mean(err_dict['w_ffe']))
    print('Character FFE: ', np.mean(err_dict['p_ffe']))


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--base_path', default='../results/vctk/', help='Base path to all conversion methods')
    parser.add_argument('--method', default='sr', help='Name of conversion type, as in folder name')
    parser.add_argument('--device', default='cuda:0', help='Torch device')
    parser.add_argument('--target_speakers', nargs='+', default=['p231', 'p239', 'p245', 'p270'], help='Target speakers for VC. If none random speakers are used')
    parser.add_argument('--batch_seconds', default=640.0, type=float, help='audio seconds per GPU batch')
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    from dissc_amd.metrics import ProsodyEvaluator
    errs = calc_errors(ProsodyEvaluator(args.device, batch_seconds=args.batch_seconds), args)
    log_results(errs, args)


if __name__ == '__main__':
    main()
