#!/usr/bin/env python3
"""AuroraCap inference on MI355X - same argument surface and stdout contract as the reference CLI
(rese1f/aurora inference.py:29-98): prints one caption string.

    python inference.py --model_path <xtuner-format dir> --visual_input clip.mp4 --num_frm 8 \
        --token_kept_ratio 0.3 --max_new_tokens 256

Tokenizer and PyAV frame decoding use the same third-party packages the reference uses; resize / crop / normalise
(bit-identical to the reference's CLIPImageProcessor call) and the three hot stages run in libaurora_hip.so.
`--synthetic` replaces checkpoint, tokenizer and video by the seeded synthetic clip of SURVEY 8d (prints ids).
"""
import argparse
import os.path as osp
import sys

import numpy as np
import torch


from aurora_amd.preprocess import read_video_pyav  # noqa: E402  (frame sampling contract of load_video.py:31-71)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    # the reference CLI's argument surface (inference.py:31-40): same flags, types and defaults
    for flag, typ, default, text in (
            ("model_path", str, "wchai/AuroraCap-7B-IMG-xtuner", "checkpoint directory (xtuner layout) or hub id"),
            ("prompt", str, "Describe the video in detail.", "instruction given to the model"),
            ("visual_input", str, "output.png", "video (.mp4) or image (.png / .jpg) file"),
            ("num_frm", int, 8, "frames sampled uniformly from a video"),
            ("token_kept_ratio", float, 0.8, "fraction of visual tokens kept by the per-layer token merge"),
            ("temperature", float, 0.0, "sampling temperature (takes effect with --do_sample; without it generation is greedy)"),
            ("top_p", float, 1.0, "nucleus mass kept by top-p sampling (takes effect with --do_sample)"),
            ("num_beams", int, 1, "beam count (only 1 is implemented)"),
            ("max_new_tokens", int, 2048, "generation budget")):
        parser.add_argument("--" + flag, type=typ, default=default, help=text)
    parser.add_argument('--host_preprocess', action='store_true', help='resize/normalise on the host with CLIPImageProcessor (PIL) instead of the HIP input stage')
    parser.add_argument('--synthetic', action='store_true', help='seeded synthetic weights / clip / prompt ids (no checkpoint needed)')
    # the reference CLI hard-codes do_sample=False (inference.py:91); sampling is this path's own switch
    parser.add_argument('--do_sample', action='store_true', help='seeded sampling with --temperature (required, > 0) / --top_p / --top_k instead of greedy decoding')
    parser.add_argument('--top_k', type=int, default=50, help='with --do_sample: keep the k most likely tokens (0 = off)')
    parser.add_argument('--seed', type=int, default=0, help='with --do_sample: seed of the counter-based generator (same seed, same caption)')
    # transformers' remedies for loops, ahead of the pick (greedy or sampled); their history is the generated tokens, not the prompt.
    # Left out, a flag falls back to the checkpoint's generation_config.json, then to off
    parser.add_argument('--repetition_penalty', type=float, default=None, help='divide (positive) / multiply (negative) the logit of every token generated so far by this (> 0; 1.0 = off)')
    parser.add_argument('--no_repeat_ngram_size', type=int, default=None, help='no n-gram of this size occurs twice in the generated tokens (0 = off)')
    parser.add_argument('--min_new_tokens', type=int, default=None, help='the EOS token cannot be picked before this many tokens (0 = off)')
    # classifier-free guidance (aurora_amd.guidance): every pick contrasts the prompt with a negative prompt that decodes beside it
    parser.add_argument('--guidance_scale', type=float, default=None, metavar='G',
                        help='contrast the caption\'s distribution with a negative prompt\'s: G * (log p - log p_neg) + log p_neg ahead of every '
                             'pick (> 0; 1.0 = off; above 1 pushes down what the language prior alone would have written)')
    parser.add_argument('--negative_prompt', default=None, metavar='TEXT',
                        help='with --guidance_scale: the negative prompt (default: --prompt without the visual input); with --synthetic there is '
                             'no tokenizer: the text is ignored and the default negative is used')
    # more questions about the same input: the vision tower runs once and the later prompts prefill only the rows behind the last visual token
    parser.add_argument('--stop', action='append', default=[], metavar='STR',
                        help='end the caption behind the token that completes this text (repeatable, at most 8 of up to 64 bytes); the text '
                             'stays in the printed caption')
    parser.add_argument('--stop_token_id', action='append', type=int, default=[], metavar='N',
                        help='end the caption behind this token id (repeatable, at most 8)')
    parser.add_argument('--extra_prompt', action='append', default=[], metavar='TEXT',
                        help='a further instruction about the same visual input (repeatable): one more caption is printed per flag, in order; '
                             'with --synthetic there is no tokenizer: the text is ignored and each flag adds a seeded prompt of its own length')
    parser.add_argument('--score', default=None, metavar='TEXT',
                        help='instead of generating: print the log-likelihood of TEXT as the answer to --prompt (the sum of its tokens\' '
                             'log-probabilities), with is_greedy (every token of TEXT is the greedy pick) and the token count; '
                             'with --synthetic there is no tokenizer: the text is ignored and a seeded answer of 8 tokens is scored')
    parser.add_argument('--logprobs', type=int, default=None, metavar='N',
                        help='after the caption: one line per generated token - id, decoded piece, log-probability under the model\'s '
                             'unmodified distribution, and its N (0 .. 8) most likely alternatives -, then their sum and exp(-mean)')
    # which patches each visual token stands for (aurora_amd.merge_map); neither flag changes the caption line
    parser.add_argument('--merge_map', default=None, metavar='OUT.npz',
                        help='write the merge map of the visual tokens: merge_map int32 [frames, gh, gw] (the kept token every patch was merged '
                             'into), sizes (patches per kept token, one row per frame), grid and token_kept_ratio')
    parser.add_argument('--merge_vis', default=None, metavar='OUT.png',
                        help='write the frames side by side with every patch filled with the mean colour of its merged group and a line '
                             'between neighbouring patches of different groups')
    # which visual tokens each generated token looked at (aurora_amd.attn_map); neither flag changes the caption line
    parser.add_argument('--attn_map', default=None, metavar='OUT.npz',
                        help='write, per generated token, its attention over the prompt (mean over layers and heads): attn_map float32 '
                             '[tokens, keys], vis_rows, visual_attention [tokens, visual tokens], visual_share [tokens] and ids')
    parser.add_argument('--attn_vis', default=None, metavar='OUT.png',
                        help='write one row of heat maps per generated token, one tile per frame: each visual token\'s attention spread '
                             'over the patches it stands for (the merge map of the same run)')
    return parser


def write_attn_outputs(args, out, output):
    """--attn_map / --attn_vis: the record `llm.generate(output_attentions=True)` returned, as an npz and as heat maps over the patch grid
    (`attn_map.to_patches` with the merge map of the same run, `attn_map.render`; host work)."""
    from aurora_amd import attn_map as AMAP
    va = out.visual_attention.numpy()
    if args.attn_map:
        with open(args.attn_map, "wb") as fh:
            np.savez(fh, attn_map=out.prompt_attention[0].numpy(), vis_rows=output["vis_rows"].numpy(), visual_attention=va,
                     visual_share=out.visual_share.numpy(), ids=out.sequences[0].numpy())
    if args.attn_vis:
        from PIL import Image
        heat = AMAP.to_patches(va, output["merge_map"].cpu().numpy())
        Image.fromarray(AMAP.render(heat, patch=max(1, 112 // heat.shape[-1]))).save(args.attn_vis)


def write_merge_outputs(args, output, pixel_values, patch):
    """--merge_map / --merge_vis: the map `model(data)` returned, as an npz and as a picture (`merge_map.render`; host work)."""
    from aurora_amd import merge_map as MM
    from aurora_amd.preprocess import CLIP_MEAN, CLIP_STD
    mp = output["merge_map"].cpu().numpy()
    szs = [s.cpu().numpy() for s in output["merge_sizes"]]
    if args.merge_map:
        width = max(len(s) for s in szs)
        sizes = np.zeros((len(szs), width), np.float32)                # slow-fast frames keep different counts: rows padded with 0
        for f, s in enumerate(szs):
            sizes[f, :len(s)] = s
        with open(args.merge_map, "wb") as fh:
            np.savez(fh, merge_map=mp, sizes=sizes, n_kept=np.array([len(s) for s in szs], np.int32),
                     grid=np.array(mp.shape[1:], np.int32), token_kept_ratio=np.float64(args.token_kept_ratio))
    if args.merge_vis:
        from PIL import Image
        px = pixel_values[0] if pixel_values.dim() == 5 else pixel_values
        px = px.float().cpu().numpy().transpose(0, 2, 3, 1)            # the normalised input frames back to 8-bit RGB
        rgb = np.clip(np.rint((px * np.asarray(CLIP_STD, np.float32) + np.asarray(CLIP_MEAN, np.float32)) * 255.0), 0, 255).astype(np.uint8)
        img = MM.render(rgb, mp, patch)
        Image.fromarray(np.concatenate(list(img), axis=1)).save(args.merge_vis)


def print_logprobs(out, tokenizer):
    """One line per generated token: `token <i> id <id> <piece> logprob <lp> top <id>:<lp> ...`; then `sum_logprob <s> perplexity <p>`."""
    ids, lps = out.sequences[0].tolist(), out.token_logprobs[0].tolist()
    piece = (lambda t: repr(str(t))) if tokenizer is None else (lambda t: repr(tokenizer.convert_ids_to_tokens(int(t))))
    for i, (t, lp) in enumerate(zip(ids, lps)):
        alts = " ".join(f"{int(a)}:{float(v)!r}" for a, v in zip(out.top_ids[0, i].tolist(), out.top_logprobs[0, i].tolist()))
        print(f"token {i} id {t} {piece(t)} logprob {float(lp)!r} top {alts}".rstrip())
    total = 0.0
    for lp in lps:
        total += float(lp)
    print(f"sum_logprob {total!r} perplexity {float(np.exp(-total / max(len(lps), 1)))!r}")


def main():
    args = build_parser().parse_args()
    if args.do_sample and not args.temperature > 0:
        sys.exit("error: --do_sample needs --temperature > 0 (the reference CLI's default temperature, 0.0, is kept: it means greedy)")
    if args.logprobs is not None and not 0 <= args.logprobs <= 8:
        sys.exit("error: --logprobs takes a number of alternatives in [0, 8]")
    if args.logprobs is not None and (args.extra_prompt or args.score is not None):
        sys.exit("error: --logprobs goes with one generated caption (not with --extra_prompt or --score)")
    want_map = args.merge_map is not None or args.merge_vis is not None
    if want_map and (args.extra_prompt or args.score is not None):
        sys.exit("error: --merge_map / --merge_vis go with one generated caption (not with --extra_prompt or --score)")
    want_attn = args.attn_map is not None or args.attn_vis is not None
    if want_attn and (args.extra_prompt or args.score is not None):
        sys.exit("error: --attn_map / --attn_vis go with one generated caption (not with --extra_prompt or --score)")
    rule_args = {k: getattr(args, k) for k in ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens") if getattr(args, k) is not None}
    try:
        from aurora_amd.logit_rules import check_logit_rules
        check_logit_rules(rule_args)
    except ValueError as e:
        sys.exit(f"error: {e}")
    try:
        from aurora_amd.guidance import check_scale
        gscale = check_scale(args.guidance_scale)
    except ValueError as e:
        sys.exit(f"error: {e}")
    if gscale is not None and args.score is not None:
        sys.exit("error: --guidance_scale goes with generated captions (not with --score)")
    try:
        from aurora_amd.stopping import check_stop
        stop = check_stop(dict(strings=args.stop, token_ids=args.stop_token_id), need_table=False)
    except ValueError as e:
        sys.exit(f"error: {e}")
    if args.stop and args.synthetic:
        sys.exit("error: --stop matches text and needs a checkpoint's tokenizer (--synthetic has none); --stop_token_id works without one")
    if stop is not None and args.score is not None:
        sys.exit("error: --stop / --stop_token_id go with generated captions (not with --score)")
    if args.num_beams != 1:
        sys.exit("error: beam search is not implemented on the MI355X path: generation is greedy or, with --do_sample, sampled (--num_beams 1)")

    from aurora_amd.model import AuroraModel, build_prompt, process_text

    if args.synthetic:
        from aurora_amd import synthetic as S
        from aurora_amd.engine import AuroraCapEngine
        cfg = S.AURORACAP_7B
        w = {"vit": S.vit_weights(cfg["vit"]), "projector": S.projector_weights(1280, 4096), "llm": S.llm_weights(cfg["llm"])}
        n_prompts = 1 + len(args.extra_prompt)
        eng = AuroraCapEngine(cfg, w, max_frames=args.num_frm, max_batch=n_prompts * (2 if gscale is not None else 1),
                              max_ctx=30 + args.num_frm * 729 + args.max_new_tokens + 64 + 3 * len(args.extra_prompt),
                              max_new_tokens=args.max_new_tokens)
        model = AuroraModel(eng, eos_token_id=None)
        data = {"pixel_values": S.frames(args.num_frm, 0).unsqueeze(0), "input_ids": torch.tensor([S.prompt_ids(args.num_frm, 0)])}
        tokenizer = None
        # the j-th extra prompt: the same ids up to the last image marker, then a seeded tail of its own length
        ids0 = S.prompt_ids(args.num_frm, 0)
        head = ids0[:len(ids0) - ids0[::-1].index(-200)]
        extra_ids = [head + np.random.default_rng(3000 + j).integers(3, 32000, size=8 + 3 * j).tolist() for j in range(len(args.extra_prompt))]
    else:
        from transformers import AutoTokenizer, CLIPImageProcessor
        if not osp.isdir(args.model_path):
            from huggingface_hub import snapshot_download
            args.model_path = snapshot_download(repo_id=args.model_path)
        # input size / patch size come from the checkpoint's own config; the reference writes the AuroraCap-7B values
        # (size=378, crop_size=378, inference.py:58-63) into its processor call, which is what the release's config says too
        from aurora_amd.checkpoint import vit_config
        vcfg = vit_config(osp.join(args.model_path, "visual_encoder"))
        image_size, patch = vcfg["image_size"], vcfg["patch_size"]
        if args.host_preprocess:      # the reference's host path (PIL); default is the bit-identical HIP input stage
            try:
                image_processor = CLIPImageProcessor.from_pretrained("laion/CLIP-ViT-bigG-14-laion2B-39B-b160k", size=image_size, crop_size=image_size)
            except OSError:           # no hub access: that repository's preprocessor_config.json holds the class defaults (OpenAI CLIP mean / std, bicubic)
                image_processor = CLIPImageProcessor(size=image_size, crop_size=image_size)

            def to_pixels(frames):
                return image_processor(list(frames), return_tensors='pt')['pixel_values'].to(dtype=torch.float16)
        else:
            from aurora_amd.preprocess import FramePreprocessor
            gpu_pre = FramePreprocessor(image=image_size)

            def to_pixels(frames):
                return gpu_pre(torch.from_numpy(np.ascontiguousarray(np.stack(list(frames)))).cuda())
        tokenizer = AutoTokenizer.from_pretrained(args.model_path, trust_remote_code=True, padding_side='right')
        data = dict()
        if args.visual_input.endswith('mp4'):
            video_frames = read_video_pyav(args.visual_input, args.num_frm)
            data["pixel_values"] = to_pixels(video_frames).unsqueeze(0)
            n_img = len(video_frames)
        elif args.visual_input.endswith('png') or args.visual_input.endswith('jpg'):
            from PIL import Image
            image = np.asarray(Image.open(args.visual_input).convert("RGB"))       # the processor's do_convert_rgb
            data["pixel_values"] = to_pixels([image])
            n_img = 1
        else:
            sys.exit("error: --visual_input must end with mp4, png or jpg")
        data["input_ids"] = process_text(build_prompt(args.prompt, n_img), tokenizer)
        extra_ids = [process_text(build_prompt(p, n_img), tokenizer)[0].tolist() for p in args.extra_prompt]
        # The engine's capacity comes from THIS request: read_video_pyav may return num_frm + 1 frames and the
        # prompt length is only known after tokenising, so size the context from the spliced length, not from the flags.
        n_text = max(sum(1 for t in ids if t != -200) for ids in [data["input_ids"][0].tolist()] + extra_ids)
        per_frame = (image_size // patch) ** 2                                      # upper bound: token_kept_ratio = 1.0 keeps all patches
        max_ctx = -(-(n_text + n_img * per_frame + args.max_new_tokens) // 64) * 64
        model = AuroraModel.from_pretrained(args.model_path, max_frames=max(n_img, 1), max_ctx=max_ctx,
                                            max_new_tokens=args.max_new_tokens, max_batch=(1 + len(extra_ids)) * (2 if gscale is not None else 1))

    model.visual_encoder.reset_tome_r(args.token_kept_ratio)
    neg_ids = None                    # the negative prompt's text ids; None = the prompt itself without its image markers
    if gscale is not None and args.negative_prompt is not None and tokenizer is not None:
        neg_ids = [t for t in process_text(build_prompt(args.negative_prompt, 0), tokenizer)[0].tolist() if t != -200]
    if args.score is not None:        # how likely is this answer: one pass over prompt + answer, the answer's rows scored
        px = data["pixel_values"][0] if data["pixel_values"].dim() == 5 else data["pixel_values"]
        ctx_ids = data["input_ids"][0].tolist()
        if tokenizer is None:
            cont_ids = np.random.default_rng(4000).integers(3, 32000, size=8).tolist()
        else:                         # the answer as the prompt's continuation: the ids the full text adds behind the prompt's
            full = process_text(build_prompt(args.prompt, n_img) + args.score, tokenizer)[0].tolist()
            cont_ids = full[len(ctx_ids):]
        r = model.loglikelihood_batch([(px, ctx_ids, cont_ids)])[0]
        print(f"loglikelihood {r['logprob']:.6f} is_greedy {r['greedy']} tokens {r['count']}")
        return
    if extra_ids:                     # several prompts about one input: one caption per prompt, in order
        px = data["pixel_values"][0] if data["pixel_values"].dim() == 5 else data["pixel_values"]
        samp = dict(temperature=args.temperature, top_p=args.top_p, top_k=args.top_k, seed=args.seed) if args.do_sample else None
        if args.stop:
            model.llm.use_tokenizer(tokenizer)
        outs = model.caption_prompts(px, [data["input_ids"][0].tolist()] + extra_ids, max_new_tokens=args.max_new_tokens, sampling=samp,
                                     **(dict(logit_rules=rule_args) if rule_args else {}), **(dict(stop=stop) if stop is not None else {}),
                                     **(dict(guidance_scale=gscale, negative_prompt=neg_ids) if gscale is not None else {}))
        for ids in outs:
            print(ids if tokenizer is None else tokenizer.batch_decode([ids], skip_special_tokens=True)[0])
        return
    if want_map or args.attn_vis is not None:        # the heat maps spread each visual token over the patches it stands for
        data["output_merge_map"] = True
    if want_attn:
        data["output_attentions"] = True
    output = model(data, mode="inference")
    if want_map:
        write_merge_outputs(args, output, data["pixel_values"], model.visual_encoder.config["patch_size"])
    sample = dict(top_k=args.top_k, seed=args.seed) if args.do_sample else {}
    cont = model.llm.generate(**output, do_sample=args.do_sample, temperature=args.temperature, top_p=args.top_p,
                              num_beams=args.num_beams, max_new_tokens=args.max_new_tokens, **sample, **rule_args,
                              **(dict(stop_strings=args.stop, tokenizer=tokenizer) if args.stop else {}),
                              **(dict(stop_token_ids=args.stop_token_id) if args.stop_token_id else {}),
                              **(dict(return_dict_in_generate=True) if args.logprobs is not None or want_attn else {}),
                              **(dict(output_logprobs=True, top_logprobs=args.logprobs) if args.logprobs is not None else {}),
                              **(dict(output_attentions=True) if want_attn else {}),
                              **(dict(guidance_scale=gscale, negative_prompt_ids=neg_ids if neg_ids is not None
                                      else [t for t in data["input_ids"][0].tolist() if t != -200]) if gscale is not None else {}))
    lp_out = None
    if want_attn:
        write_attn_outputs(args, cont, output)
    if args.logprobs is not None or want_attn:
        lp_out, cont = (cont if args.logprobs is not None else None), cont.sequences
    if tokenizer is None:
        print(cont[0].tolist())
    else:
        print(tokenizer.batch_decode(cont, skip_special_tokens=True)[0])
    if lp_out is not None:
        print_logprobs(lp_out, tokenizer)


if __name__ == "__main__":
    main()
