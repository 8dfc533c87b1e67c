"""TurboTranscriber: the drop-in for the ASR callable the reference builds and calls.

Reference: AudioProcessingPipeline.load_transcription_model stores
`transformers.pipeline("automatic-speech-recognition", ...)` in `self.transcription_model`
(/root/reference/vocalis/core/audio_pipeline.py:171-208) and `transcribe` calls it as
    outputs = self.transcription_model(audio_path, chunk_length_s=60, batch_size=512|32,
                                       stride_length_s=5, generate_kwargs={"task": task},
                                       return_timestamps=return_timestamps)      (:351-358)
TurboTranscriber.__call__ accepts the same arguments and returns the same dict
({"text": str, "chunks": [{"timestamp": (start, end), "text": str}, ...]}), following
AutomaticSpeechRecognitionPipeline preprocess / _forward / postprocess
($TF/pipelines/automatic_speech_recognition.py:345-710) with every numeric stage on the GPU engine.
"""
from __future__ import annotations

import ctypes
import os
from types import SimpleNamespace
from typing import Any, Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib, audio, dist, seqbias
from .config import PRESETS, GenerationSettings, WhisperDims
from .engine import WhisperEngine
from .engine_f32 import WhisperEngineF32
from .frontend import CHUNK_SAMPLES, SAMPLE_RATE, Window, chunk_windows, time_precision
from .segments import FallbackConfig, pad_right
from .tokenizer import LANGUAGE_NAMES, WhisperVocab, collate_word_timestamps, decode_asr, mean_logprob
from .weights import build_weights

_NAME_TO_CODE = {v: k for k, v in LANGUAGE_NAMES.items()}

# AutomaticSpeechRecognitionPipeline._default_generation_config ($TF/pipelines/automatic_speech_recognition.py:160-163)
PIPELINE_DEFAULT_NUM_BEAMS = 5
PIPELINE_DEFAULT_MAX_NEW_TOKENS = 256
_GLOBAL_DEFAULT_MAX_LENGTH = 20  # GenerationConfig's own max_length default


def _alternatives_arg(k, word: bool, name: str) -> int:
    """return_alternatives / alternatives checked: 0 (off) or 1..TW_TOPK_MAX (8), and only with word timestamps."""
    top = _lib.TW_TOPK_MAX
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) <= top:
        raise ValueError(f"`{name}` must be an integer from 0 (off) to {top}, got {k!r}")
    if k and not word:
        raise ValueError(f"`{name}` needs return_timestamps=\"word\": the alternatives are returned per word")
    return int(k)


def resolve_decode(gen: GenerationSettings, gk: Dict[str, Any]) -> Dict[str, Any]:
    """The decode the HF ASR pipeline runs when called the way the reference calls it.

    Pipeline.__init__ ($TF/pipelines/base.py:887-908) prepares the pipeline's generation config from its class
    default {max_new_tokens: 256, num_beams: 5} through `_prepare_generation_config` ($TF/generation/utils.py:
    1771-1830): values the default sets are kept, only unset ones are filled from the checkpoint's
    generation_config.json. So `num_beams` is 5 whatever the checkpoint says, unless the call passes it in
    generate_kwargs (the reference passes only {"task": task}, vocalis/core/audio_pipeline.py:351-358). The pipeline's
    max_new_tokens=256 is then dropped in favour of the checkpoint's max_length when that is set and differs from
    GenerationConfig's global default 20 (Whisper checkpoints set 448). Pinned by tests/golden/defaults.json, made
    by transformers itself (tests/golden/make_golden.py defaults).

    Returns {"num_beams", "max_new_tokens"} (max_new_tokens None = bounded by max_length)."""
    nb = gk.get("num_beams")
    mnt = gk.get("max_new_tokens")
    if mnt is None and "max_new_tokens" not in gk:
        ml = gen.max_length if gen.max_length_set else _GLOBAL_DEFAULT_MAX_LENGTH
        mnt = None if ml != _GLOBAL_DEFAULT_MAX_LENGTH else PIPELINE_DEFAULT_MAX_NEW_TOKENS
    return {"num_beams": int(nb) if nb is not None else PIPELINE_DEFAULT_NUM_BEAMS, "max_new_tokens": mnt}


def _with_prefix(e: Exception, prefix: str) -> Exception:
    """An exception of e's type whose message is e's behind `prefix` (e itself, its message rewritten, where the
    type cannot be built from one string)."""
    try:
        return type(e)(prefix + str(e))
    except Exception:
        e.args = (prefix + str(e),)
        return e


class TurboTranscriber:
    """Callable with the HF ASR pipeline signature, backed by WhisperEngine (HIP)."""

    def __init__(self, engine: WhisperEngine, vocab: WhisperVocab, sampling_rate: int = SAMPLE_RATE):
        self.engine = engine
        self.vocab = vocab
        self.sampling_rate = sampling_rate
        self.gen = engine.gen
        # A share of n <= max_batch windows is split into two sub-batches when n >= 2 * sub_batch_min, so that
        # run_batches' two-slot pipeline encodes the second beside the first one's decode (a single 1-h request on
        # 8 GPUs gives each rank 15 windows: one batch, no overlap). None: never split (see DESIGN.md §C3 for the
        # measured trade: the decode step is latency-bound, so two decodes of 8 cost about two of 15).
        self.sub_batch_min: Optional[int] = None
        self.sample_seed = 0  # key of the fallback sampler (generate_kwargs "seed" overrides it per call)
        self._staging = None  # two pinned host buffers for the per-batch waveform upload (host-array inputs)

    # -------------------------------------------------------------- construction
    @staticmethod
    def from_pretrained(model: str = "large-v3-turbo", checkpoint: Optional[str] = None, seed: int = 1234,
                        max_batch: int = 24, device: str = "cuda", use_graphs: bool = True,
                        max_beams: int = PIPELINE_DEFAULT_NUM_BEAMS, enc_fp8: Optional[bool] = None,
                        precision: str = "bf16", fused_decode: bool = False) -> "TurboTranscriber":
        """`model`: a preset name (synthetic seeded weights) or, via `checkpoint`, a LOCAL Hugging Face
        Whisper directory (config.json, *.safetensors, vocab.json, generation_config.json). max_beams: decoder rows
        per window (the callable's default decode is beam-5, as the HF pipeline's; 1 = greedy-only engine). enc_fp8:
        run the encoder projections on MX fp8 (BASELINE config 5; default: env TW_ENC_FP8). precision: "bf16" (the
        engine's default arithmetic) or "fp32" (every operand, activation and cache f32: BASELINE configs[0], the
        reference's torch_dtype=torch.float32 load; WhisperEngineF32). fused_decode: greedy / sampled decode passes of
        at most 4 rows run the decoder's layers as one persistent launch (WhisperEngine.dec_fused_alone; 9-14 % less
        per step at 1-4 rows, rounding like, not bit-equal to, the default launch chain)."""
        if precision not in ("bf16", "fp32"):
            raise ValueError(f"precision {precision!r}: 'bf16' or 'fp32'")
        if checkpoint is None and model not in PRESETS and os.path.isdir(model):
            checkpoint = model
        if checkpoint is not None:
            dims = _dims_from_checkpoint(checkpoint)
            gen = GenerationSettings.from_checkpoint(checkpoint, dims)
            vocab = WhisperVocab.from_checkpoint(checkpoint, gen.special)
        else:
            key = model.split("/")[-1].replace("whisper-", "")
            if key not in PRESETS:
                raise ValueError(f"unknown model {model!r}: give a preset ({sorted(PRESETS)}) or a local checkpoint dir")
            dims = PRESETS[key]
            gen = GenerationSettings.default(dims)
            vocab = WhisperVocab.synthetic(gen.special)
        f32 = precision == "fp32"
        weights = build_weights(dims, seed=seed, checkpoint=checkpoint, dtype=torch.float32 if f32 else torch.bfloat16)
        cls = WhisperEngineF32 if f32 else WhisperEngine
        eng = cls(weights, gen, max_batch=max_batch, device=device, use_graphs=use_graphs, max_beams=max_beams,
                  enc_fp8=enc_fp8)
        eng.dec_fused_alone = bool(fused_decode)
        return TurboTranscriber(eng, vocab)

    # -------------------------------------------------------------- call
    def close(self) -> None:
        """Release the engine (WhisperEngine.close) and the pinned staging buffers; the callable is unusable after."""
        self._staging = None
        if self.engine is not None:
            self.engine.close()

    def __enter__(self) -> "TurboTranscriber":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __call__(self, inputs: Union[str, bytes, np.ndarray, dict, list], *, chunk_length_s: float = 0,
                 stride_length_s=None, batch_size: int = 1, generate_kwargs: Optional[Dict[str, Any]] = None,
                 return_timestamps: Union[bool, str] = False, return_language: bool = False,
                 return_confidence: bool = False, return_alternatives: int = 0,
                 **kwargs) -> Union[dict, List[dict]]:
        """The HF ASR pipeline call. A `list` of inputs returns the list of their results, in order, with the
        windows of all inputs sharing engine batches (_call_list; any other iterable is refused as before).
        return_confidence (extension): the log-probability of every generated token
        under its step's processed scores (WhisperEngine.generate(token_logprobs=True)) rides through the stitching
        and comes out as each word's "probability" (return_timestamps="word": the mean of exp(lp) over the word's
        tokens, openai-whisper's definition), each chunk's "avg_logprob" (return_timestamps=True) or the result's
        "avg_logprob"; text, timestamps and chunks are those of the call without it. last_window_pass_logprobs then
        sits beside last_window_passes. return_alternatives = k (extension, 1..8, with return_timestamps="word"):
        every word dict gains "alternatives", one list per token of the word, each up to k dicts {"id", "text",
        "logprob"} — the model's k best candidates at that token under the step's processed scores, best first
        (WhisperEngine.generate(top_alternatives=k)); every other value is that of the call without it."""
        word = return_timestamps == "word"
        conf = bool(return_confidence)
        n_alt = _alternatives_arg(return_alternatives, word, "return_alternatives")
        if return_timestamps == "char":
            raise ValueError("Whisper cannot return `char` timestamps, only word level or segment level timestamps.")
        gk = dict(generate_kwargs or {})
        gk.update({k: kwargs.pop(k) for k in list(kwargs) if k in ("max_new_tokens", "language", "task", "num_beams")})
        dec = resolve_decode(self.gen, gk)  # as shipped: beam-5, bounded by max_length (see resolve_decode)
        gk.pop("num_beams", None)
        gk.pop("max_new_tokens", None)
        num_beams = dec["num_beams"]
        if num_beams < 1 or num_beams > 8:
            raise ValueError(f"num_beams={num_beams}: the engine supports 1 (greedy) to 8 beams")
        task = gk.pop("task", None)
        language = gk.pop("language", None)
        max_new_tokens = dec["max_new_tokens"]
        # extension (not a transformers generate kwarg): bound the seek loop to this many passes per window
        max_passes = gk.pop("max_passes", None)
        # prompt every seek pass after a window's first with its previous segments (generate()'s
        # condition_on_prev_tokens; the batch then shapes results through the left padding, so batch_size is kept)
        cond = bool(gk.pop("condition_on_prev_tokens", None) or False)
        # generate()'s initial prompt (<|startofprev|> + text tokens, WhisperProcessor.get_prompt_ids) and where it
        # conditions (first-segment / all-segments)
        prompt = {}
        if gk.get("prompt_ids") is not None:
            pid = gk.pop("prompt_ids")
            pid = pid.tolist() if hasattr(pid, "tolist") else list(pid)
            prompt = {"prompt_ids": [int(t) for t in np.asarray(pid).reshape(-1)],
                      "prompt_condition_type": gk.pop("prompt_condition_type", None)}
        gk.pop("prompt_ids", None)
        if "prompt_condition_type" in gk:
            prompt.setdefault("prompt_condition_type", gk.pop("prompt_condition_type"))
        # (_set_prompt_condition_type's checks, generation_whisper.py:1732-1748, before any work is queued)
        pct = prompt.get("prompt_condition_type") or "first-segment"
        if pct not in ("first-segment", "all-segments"):
            raise ValueError(f"`prompt_condition_type={pct} does not exist. Make sure to set `prompt_condition_type` "
                             "to one of first-segment, all-segments")
        if pct == "all-segments" and not cond:
            raise ValueError("Make sure to set `condition_on_prev_tokens=True` when setting "
                             "`prompt_condition_type='all-segments'`.")
        if "prompt_ids" not in prompt:
            prompt = {}
        fallback = self._fallback_config(gk)
        hist = self._history_options(gk, vocab=getattr(getattr(self.engine, "d", None), "vocab", None))
        if gk:
            raise ValueError(f"generate_kwargs not supported by this engine: {sorted(gk)}")
        st = self.gen.special
        if not st.is_multilingual and (task is not None or language is not None):
            raise ValueError("Cannot specify `task` or `language` for an English-only model.")

        o = SimpleNamespace(word=word, conf=conf, n_alt=n_alt, task=task, language=language, num_beams=num_beams,
                            max_new_tokens=max_new_tokens, max_passes=max_passes, cond=cond, prompt=prompt,
                            fallback=fallback, hist=hist, batch_size=batch_size, chunk_length_s=chunk_length_s,
                            stride_length_s=stride_length_s, return_timestamps=return_timestamps,
                            return_language=return_language)
        if isinstance(inputs, list):  # the pipeline's list call: a list of results, engine batches shared
            return self._call_list(inputs, o)

        rank, world = dist.world()
        sharded = dist.collective_path()  # (world > 1, or a forced collective in a world of one)
        dev = getattr(self.engine, "device", None)
        wav, load_err = None, None
        if rank == 0:
            try:
                wav = audio.load_input(inputs, self.sampling_rate, dev)
            except Exception as e:  # raised below, after the other ranks have been told (no rank left waiting)
                load_err = e
        if sharded:  # SPMD: every rank calls with the same arguments; rank 0 decoded the input
            # (the waveform stays in device memory: each rank copies its windows out of it on the GPU)
            wav = dist.broadcast_waveform(wav, failed=load_err is not None, as_tensor=True)
        if load_err is not None:
            raise load_err
        if chunk_length_s:
            windows = list(chunk_windows(len(wav), chunk_length_s, stride_length_s, self.sampling_rate))
            if not windows:  # an empty input: the pipeline's chunk iterator yields nothing and its first next()
                # raises StopIteration (tests/golden/edge.json), which transcribe() reports as "Transcription error: "
                raise StopIteration
            with_stride = True
        elif len(wav) > CHUNK_SAMPLES:  # long-form: one sequential generate() over the whole input (asr:450-457)
            return self._long_form(wav, **self._long_form_options(o))
        else:
            windows = [Window(0, len(wav), 0, 0, True)]
            with_stride = False
        model_outputs = self._window_outputs(o, wav, windows, with_stride, sharded)
        kw = self._stitch_options(o)
        # sharded: every rank stitches its own windows and the pieces are merged (dist.stitch_sharded: the serial
        # _decode_asr result, without rank 0 walking every window of the call)
        text, optional = (dist.stitch_sharded(self.vocab, model_outputs, **kw) if sharded else
                          decode_asr(self.vocab, model_outputs, **kw))
        return {"text": text, **optional}

    # the per-window records of the last call (transcribe_windows / _long_form), flat over a list call's windows
    _WINDOW_RECORDS = ("last_window_langs", "last_window_passes", "last_window_prefixes",
                       "last_window_token_timestamps", "last_window_pass_logprobs", "last_window_token_logprobs",
                       "last_window_token_alternatives")

    def _call_list(self, inputs: list, o) -> List[dict]:
        """The list call (Pipeline.__call__ on a list, $TF/pipelines/base.py:1270-1278): one result per input, in
        order, every call option applied to every input. Rank 0 decodes every input into one arena (the 16 kHz
        waveforms, concatenated; device memory on a GPU engine, uploaded once). With chunk_length_s the windows of
        all inputs form one flat list with arena-absolute starts and go through the engine once, so engine batches
        (and, where batch composition shapes results, the batch_size groups) cross input boundaries as the
        pipeline's DataLoader batches do; every input's windows are then stitched on their own. Without it the
        inputs of at most 30 s are one window each and share batches, and a longer input runs through _long_form
        alone (the pipeline's result at batch_size=1). An empty element raises ValueError (transformers returns
        too few results there). last_input_windows: per input (first window, windows) into the flat
        last_window_* records (a long-form input holds one record, its passes)."""
        if not inputs:
            return []
        rank, _ = dist.world()
        sharded = dist.collective_path()
        sr = self.sampling_rate
        dev = getattr(self.engine, "device", None)
        waves, load_err = [], None
        if rank == 0:
            try:
                limit, total = audio.max_audio_seconds() * sr, 0
                for i, x in enumerate(inputs):
                    try:
                        w = audio.load_input(x, sr, dev)
                    except Exception as e:
                        named = _with_prefix(e, f"inputs[{i}]: ")
                        raise named from (e if named is not e else None)
                    if len(w) == 0:
                        raise ValueError(f"inputs[{i}] is empty")
                    total += len(w)
                    if total > limit:
                        raise ValueError(f"inputs[0..{i}] hold {total / sr:.1f} s, more than TW_MAX_AUDIO_S="
                                         f"{audio.max_audio_seconds():g} s in one call: split the list")
                    waves.append(w)
            except Exception as e:  # raised below, after the other ranks have been told (no rank left waiting)
                load_err = e
        arena = None if load_err is not None or rank != 0 else \
            np.concatenate([np.ascontiguousarray(w, np.float32) for w in waves])
        lengths = [len(w) for w in waves]
        if sharded:  # SPMD: every rank calls with a list of the same length; rank 0 decoded it
            lengths = dist.broadcast_lengths(lengths, len(inputs), failed=load_err is not None)
            if load_err is None:
                arena = dist.broadcast_waveform(arena, as_tensor=True)
        if load_err is not None:
            raise load_err
        if not sharded and getattr(dev, "type", None) == "cuda":  # one upload; every batch is gathered out of it
            arena = torch.from_numpy(arena).to(dev)
            torch.cuda.current_stream(dev).synchronize()
        offs = np.cumsum([0] + lengths).tolist()
        kw = self._stitch_options(o)
        results: List[Optional[dict]] = [None] * len(inputs)
        records: List[Optional[Dict[str, list]]] = [None] * len(inputs)  # per input its slice of every last_window_*
        flat: List[Window] = []
        spans: Dict[int, tuple] = {}  # input -> (first, count) in `flat`
        long_inputs: List[int] = []
        for i, n in enumerate(lengths):
            if o.chunk_length_s:
                ws = [w._replace(start=w.start + offs[i])
                      for w in chunk_windows(n, o.chunk_length_s, o.stride_length_s, sr)]
            elif n > CHUNK_SAMPLES:
                long_inputs.append(i)
                continue
            else:
                ws = [Window(offs[i], n, 0, 0, True)]
            spans[i] = (len(flat), len(ws))
            flat.extend(ws)
        for name in self._WINDOW_RECORDS:
            setattr(self, name, [])
        if flat:
            outs = self._window_outputs(o, arena, flat, bool(o.chunk_length_s), sharded)
            r, world = dist.world()
            lo, hi = dist.shard_range(len(flat), world, r) if sharded else (0, len(flat))
            for i, (first, count) in spans.items():
                text, optional = decode_asr(self.vocab, outs[first: first + count], **kw)
                results[i] = {"text": text, **optional}
                # (under a collective path the records are this rank's shard of the flat list, as in a single call)
                a, b = max(first, lo) - lo, max(min(first + count, hi), lo) - lo
                records[i] = {name: getattr(self, name)[a: b] for name in self._WINDOW_RECORDS}
        for i in long_inputs:  # each alone, as a long-form single call (every rank computes it)
            for name in self._WINDOW_RECORDS:
                setattr(self, name, [])
            results[i] = self._long_form(arena[offs[i]: offs[i + 1]], **self._long_form_options(o))
            records[i] = {name: list(getattr(self, name)) for name in self._WINDOW_RECORDS}
        self.last_input_windows = []
        merged: Dict[str, list] = {name: [] for name in self._WINDOW_RECORDS}
        first = 0
        for i, rec in enumerate(records):  # (windows of the whole call, also where the records are a rank's shard)
            count = spans[i][1] if i in spans else len(rec["last_window_passes"])
            self.last_input_windows.append((first, count))
            first += count
            for name in self._WINDOW_RECORDS:
                merged[name].extend(rec[name])
        for name, v in merged.items():
            setattr(self, name, v)
        return results

    @staticmethod
    def _long_form_options(o) -> Dict[str, Any]:
        """_long_form's keyword arguments for a call's options."""
        return dict(task=o.task, language=o.language, return_timestamps=o.return_timestamps,
                    return_language=o.return_language, max_new_tokens=o.max_new_tokens, num_beams=o.num_beams,
                    max_passes=o.max_passes, fallback=o.fallback, condition=o.cond, prompt=o.prompt, history=o.hist,
                    confidence=o.conf, alternatives=o.n_alt)

    def _stitch_options(self, o) -> Dict[str, Any]:
        """decode_asr's keyword arguments for a call's options."""
        return dict(return_timestamps="word" if o.word else bool(o.return_timestamps),
                    return_language=o.return_language,
                    time_precision=time_precision(self.engine.d.max_source_positions),
                    **({"confidence": True} if o.conf else {}), **({"alternatives": True} if o.n_alt else {}))

    def _window_outputs(self, o, wav, windows: Sequence[Window], with_stride: bool, sharded: bool) -> List[dict]:
        """The windows of a call (of one input, or of every input of a list call: their `start` indexes `wav`)
        through the engine, sharded over the ranks under a collective path: one model-output dict per window, as
        decode_asr reads them ("tokens", "stride" with with_stride, the per-token lanes the call's options ask for)."""
        word, conf, n_alt, cond, fallback, num_beams = o.word, o.conf, o.n_alt, o.cond, o.fallback, o.num_beams
        lang_id = self._lang_id(o.language)

        def run(w, ws):
            base = windows.index(ws[0]) if ws else 0  # this shard's first global window (the sampler's row keys)
            # (batch composition shapes results with word timestamps — standardised over the padded batch —, with
            # conditioned prompts — their left padding — and with beams under the fallback — a sampling round turns the
            # rest of that generate() call greedy —, so batch_size is kept there)
            grouped = word or cond or (fallback.active and num_beams > 1)
            kw = dict(task=o.task, lang_id=lang_id, return_timestamps=bool(o.return_timestamps) or word,
                      max_new_tokens=o.max_new_tokens, num_beams=num_beams, max_passes=o.max_passes,
                      **({"fallback": fallback, "window_base": base} if fallback.active else {}),
                      **({"condition_on_prev_tokens": True} if cond else {}),
                      **({"prompt": o.prompt} if o.prompt else {}),
                      **({"history": o.hist} if o.hist else {}),
                      **({"group": o.batch_size} if grouped else {}),
                      **({"token_logprobs": True} if conf else {}),
                      **({"top_alternatives": n_alt} if n_alt else {}))
            if word:  # token times ride along as floats after the tokens (one all-gather carries both)
                nf = [-(-min(x.length, CHUNK_SAMPLES) // 160) for x in ws]
                toks = self.transcribe_windows(w, ws, word_timestamps=True, num_frames=nf, **kw)
                lanes = [self.last_window_token_timestamps]
            else:
                toks = self.transcribe_windows(w, ws, **kw)
                lanes = []
            if conf:  # the log-probabilities ride the same way (0.0 beside the batch's right padding)
                lanes.append([list(lp) + [0.0] * (len(t) - len(lp))
                              for t, lp in zip(toks, self.last_window_token_logprobs)])
            if n_alt:  # 2k more lanes: slot j's ids (exact in f32) and log-probabilities; empty slots -1 / -inf
                for j in range(n_alt):
                    for f, empty in ((0, -1.0), (1, float("-inf"))):
                        lanes.append([[float(a[j][f]) if j < len(a) else empty for a in alts]
                                      + [empty] * (len(t) - len(alts))
                                      for t, alts in zip(toks, self.last_window_token_alternatives)])
            return [tuple(x) for x in zip(toks, *lanes)] if lanes else toks

        # one window shard per rank + one all-gather of the token arrays (twamd.dist); plain call on 1 GPU
        n_lanes = int(word) + int(conf) + 2 * n_alt
        outputs = dist.transcribe_sharded(run, wav, windows, timed=n_lanes) if sharded else run(wav, windows)
        model_outputs = []
        for w, toks in zip(windows, outputs):
            mo = {}
            if n_lanes:
                toks, *fl = toks
                if word:
                    mo["token_timestamps"] = fl[0]
                if conf:
                    mo["token_logprobs"] = fl[int(word)]
                if n_alt:
                    al = fl[n_lanes - 2 * n_alt:]
                    mo["token_alternatives"] = [[[int(al[2 * j][n]), al[2 * j + 1][n]] for j in range(n_alt)
                                                 if al[2 * j][n] >= 0] for n in range(len(toks))]
            mo["tokens"] = toks
            if with_stride:
                sr = self.sampling_rate
                mo["stride"] = (w.length / sr, w.stride_left / sr, w.stride_right / sr)
            model_outputs.append(mo)
        return model_outputs

    def align(self, inputs: Union[str, bytes, np.ndarray, dict], chunks: Sequence[dict], *,
              language: Optional[str] = None, task: Optional[str] = None, batch_size: Optional[int] = None,
              return_language: bool = False, alternatives: int = 0) -> dict:
        """Forced alignment (extension): when each word of a GIVEN transcript was said, and how strongly the model
        agrees that it was. chunks: [{"timestamp": (t0, t1), "tokens": [text token ids]}, ...] — the callable's chunk
        schema with token ids for text (t1 None: the end of the input); every chunk is one window of at most 30 s,
        its samples zero padded, teacher-forced through the decoder (WhisperEngine.force_pass) with the
        <|notimestamps|> prompt. Returns {"text", "chunks": word dicts as return_timestamps="word" builds them (times
        shifted by the chunk's t0, "probability" as return_confidence defines it), "chunk_avg_logprob": per input
        chunk the mean log-probability of its text tokens, None for an empty chunk}. Every argument is checked before
        any GPU work; a chunk without tokens is not run. No prompts, no history processors, not sharded.
        alternatives = k (1..8): every word dict gains "alternatives" as return_alternatives defines it, from
        force_pass's raw-logit lists — the model's own k best candidates at every given token; a given token missing
        from its list was not among them."""
        st = self.gen.special
        n_alt = _alternatives_arg(alternatives, True, "alternatives")
        if not st.is_multilingual and (task is not None or language is not None):
            raise ValueError("Cannot specify `task` or `language` for an English-only model.")
        if dist.collective_path():
            raise RuntimeError("align is not sharded: call it in a single process")
        eng, sr = self.engine, self.sampling_rate
        lang_id = self._lang_id(language)
        tail = eng.prompt_tail(task, return_timestamps=False, language_given=lang_id is not None)
        limit = eng.max_new_for(eng._prompt_len(tail))
        for i, c in enumerate(chunks):  # what needs no audio is checked before the input is even decoded
            t0, t1 = c["timestamp"]
            if not 0 <= float(t0) or (t1 is not None and not float(t0) < float(t1)):
                raise ValueError(f"align: chunk {i}: timestamp ({t0}, {t1}) needs 0 <= start < end")
            if t1 is not None and float(t1) - float(t0) > CHUNK_SAMPLES / SAMPLE_RATE + 1e-9:
                raise ValueError(f"align: chunk {i}: {float(t1) - float(t0):.3f} s is longer than one 30 s window")
            if any(not 0 <= int(t) < st.eot for t in c["tokens"]):
                raise ValueError(f"align: chunk {i}: token ids must be text tokens, below <|endoftext|> ({st.eot})")
            if len(c["tokens"]) + 1 > limit:
                raise ValueError(f"align: chunk {i}: {len(c['tokens'])} tokens and <|endoftext|> exceed the {limit} "
                                 "positions the decoder has after the prompt")
        wav = audio.load_input(inputs, sr, getattr(eng, "device", None))
        if torch.is_tensor(wav):
            wav = wav.float().cpu().numpy()
        total = len(wav)
        spans: List[Optional[tuple]] = []  # per chunk (first sample, samples, t0, tokens), None without tokens
        for i, c in enumerate(chunks):
            t0, t1 = c["timestamp"]
            t0 = float(t0)
            t1 = total / sr if t1 is None else float(t1)
            toks = [int(t) for t in c["tokens"]]
            if not (0 <= t0 < t1 and t1 <= total / sr + 1e-9):
                raise ValueError(f"align: chunk {i}: timestamp ({t0}, {t1}) is not inside the input's "
                                 f"{total / sr:.3f} s with 0 <= start < end")
            if t1 - t0 > CHUNK_SAMPLES / SAMPLE_RATE + 1e-9:  # (an end of None: known only now)
                raise ValueError(f"align: chunk {i}: {t1 - t0:.3f} s is longer than one 30 s window")
            s0 = min(int(round(t0 * sr)), total - 1)
            n = max(1, min(int(round(t1 * sr)), total, s0 + CHUNK_SAMPLES) - s0)
            spans.append((s0, n, t0, toks) if toks else None)
        run = [i for i, s in enumerate(spans) if s is not None]
        B = eng.max_batch if batch_size is None else max(1, min(int(batch_size), eng.max_batch))
        results: Dict[int, tuple] = {}  # chunk -> (language id, token times, token log-probabilities)
        for b0 in range(0, len(run), B):
            part = run[b0: b0 + B]
            host = self._host_staging(0, len(part))
            for j, i in enumerate(part):
                s0, n = spans[i][:2]
                host[j, :n] = torch.from_numpy(np.ascontiguousarray(wav[s0: s0 + n], np.float32))
                host[j, n:] = 0
            eng.wave[: len(part)].copy_(host)
            eng.logmel(len(part))
            eng.encode(len(part), row_map=False, seek=False)
            res = eng.force_pass(len(part), tail, None if lang_id is None else [lang_id] * len(part),
                                 [spans[i][3] for i in part], num_frames=[-(-spans[i][1] // 160) for i in part],
                                 **({"top_alternatives": n_alt} if n_alt else {}))
            for j, i in enumerate(part):
                results[i] = (res.lang_ids[j] if res.lang_ids else None, res.token_ts[j], res.token_lp[j],
                              res.token_alt[j] if n_alt else None)
        P = eng._prompt_len(tail)
        words: List[dict] = []
        avg: List[Optional[float]] = []
        for i, s in enumerate(spans):
            if s is None:
                avg.append(None)
                continue
            lang, ts, lp, alts = results[i]
            t0, toks = s[2], s[3]
            # the word path of AsrStitcher.feed: a token spans the previous token's time to its own
            pairs = [(round(float(ts[P + k - 1]) + t0, 2), round(float(ts[P + k]) + t0, 2)) for k in range(len(toks))]
            name = None if lang is None else LANGUAGE_NAMES.get(self.vocab.id_to_token[lang][2:-2])
            words.extend(collate_word_timestamps(self.vocab, toks, pairs, name, return_language,
                                                 token_logprobs=lp[: len(toks)],
                                                 token_alternatives=alts[: len(toks)] if n_alt else None))
            avg.append(mean_logprob(lp[: len(toks)]))
        text = "".join(self.vocab.decode(s[3]) for s in spans if s is not None)
        return {"text": text, "chunks": words, "chunk_avg_logprob": avg}

    def _lang_id(self, language: Optional[str]) -> Optional[int]:
        if language is None:
            return None
        code = language.lower()
        code = _NAME_TO_CODE.get(code, code)
        tok = f"<|{code}|>"
        lt = self.gen.special.lang_to_id()
        if tok not in lt:
            raise ValueError(f"Unsupported language: {language}.")
        return lt[tok]

    def _long_form(self, wav, *, task, language, return_timestamps, return_language, max_new_tokens, num_beams,
                   max_passes, fallback, condition=False, prompt=None, history=None, confidence=False,
                   alternatives=0) -> dict:
        """An input longer than 30 s without chunk_length_s: the pipeline hands generate() the features of the whole
        input (feature extractor with truncation=False, padding="longest", $TF/pipelines/automatic_speech_recognition
        .py:450-457) and generate() runs its seek loop over all of them (generation_whisper.py:647-968: is_shortform
        False, max_frames = the input's frames, every pass the 30-s segment at seek, zero padded). One chunk, no
        stride; every rank computes it (nothing to shard: each pass depends on the previous one's seek)."""
        # (the pipeline never passes return_timestamps=False on to generate(), asr:506-508, so generate() switches
        # timestamps on for a long-form input instead of raising; the text is then decoded without them)
        word = return_timestamps == "word"
        eng = self.engine
        lang_id = self._lang_id(language)
        x = wav if torch.is_tensor(wav) else torch.from_numpy(np.ascontiguousarray(wav, np.float32))
        eng.set_long_input(x)
        try:
            kw = {"fallback": fallback} if fallback.active else {}
            kw.update(prompt or {})
            kw.update(history or {})
            if word:  # num_frames: the feature extractor's attention mask, one per hop (_set_num_frames)
                kw.update(word_timestamps=True, num_frames=[-(-int(x.shape[0]) // 160)])
            if confidence:
                kw.update(token_logprobs=True)
            if alternatives:
                kw.update(top_alternatives=alternatives)
            toks = eng.generate(1, task=task, lang_ids=None if lang_id is None else [lang_id],
                                max_new_tokens=max_new_tokens, return_timestamps=True, num_beams=num_beams,
                                max_passes=max_passes, condition_on_prev_tokens=condition, **kw)[0]
        finally:
            eng.set_long_input(None)
        self.last_window_langs = list(eng.last_langs)
        self.last_window_passes = list(eng.last_passes)
        self.last_window_prefixes = list(eng.last_pass_prefixes)
        out = {"tokens": toks}
        if word:
            self.last_window_token_timestamps = list(eng.last_token_timestamps)
            out["token_timestamps"] = eng.last_token_timestamps[0]
        if confidence:
            self.last_window_pass_logprobs = list(eng.last_pass_logprobs)
            self.last_window_token_logprobs = list(eng.last_token_logprobs)
            out["token_logprobs"] = eng.last_token_logprobs[0]
        if alternatives:
            self.last_window_token_alternatives = list(eng.last_token_alternatives)
            out["token_alternatives"] = eng.last_token_alternatives[0]
        text, optional = decode_asr(self.vocab, [out], return_timestamps="word" if word else bool(return_timestamps),
                                    return_language=return_language,
                                    time_precision=time_precision(self.engine.d.max_source_positions),
                                    **({"confidence": True} if confidence else {}),
                                    **({"alternatives": True} if alternatives else {}))
        return {"text": text, **optional}

    def transcribe_windows(self, wav: np.ndarray, windows: Sequence[Window], task: Optional[str],
                           lang_id: Optional[int], return_timestamps: bool,
                           max_new_tokens: Optional[int] = None, num_beams: int = 1, word_timestamps: bool = False,
                           num_frames: Optional[Sequence[int]] = None, group: Optional[int] = None,
                           max_passes: Optional[int] = None, fallback: Optional[FallbackConfig] = None,
                           window_base: int = 0, condition_on_prev_tokens: bool = False,
                           prompt: Optional[dict] = None, history: Optional[dict] = None,
                           token_logprobs: bool = False, top_alternatives: int = 0) -> List[List[int]]:
        """Log-mel + generate for every window; returns per-window token sequences (generate() output,
        right-padded with the pad token within each engine batch, as the HF batch output is). Batches of
        max_batch windows go through WhisperEngine.run_batches: batch k+1 is encoded while batch k decodes.

        group: windows per engine batch when the batch's composition changes results. That is the case for
        word timestamps, whose per-pass standardisation runs over the padded batch, and for
        condition_on_prev_tokens, whose prompts are left padded to the batch's longest, so the pipeline's
        `batch_size` (its DataLoader batch, $TF/pipelines/base.py:1319-1339) is honoured there; segment-level
        tokens are per-window results, so batching is then only a schedule: the windows are cut into near-equal
        batches of at most max_batch (and into two when sub_batch_min says so).

        history: generate()'s repetition_penalty / no_repeat_ngram_size / length_penalty (those that are set), handed
        to every batch's generate(): per-pass token histories, so the results stay per-window.

        token_logprobs: every batch's generate() also records the tokens' log-probabilities
        (last_window_pass_logprobs beside last_window_passes, last_window_token_logprobs beside the returned tokens,
        unpadded). top_alternatives: likewise every token's alternatives (last_window_token_alternatives).

        wav: a host array (staged and uploaded batch by batch), or a torch tensor: in GPU memory (a rank's copy of
        the broadcast waveform, a list call's arena) every batch's rows are gathered out of it by one
        tw_gather_windows launch; a CPU tensor (gloo) is sliced."""
        eng = self.engine
        if group:
            B = max(1, min(int(group), eng.max_batch))
            sizes = [min(B, len(windows) - b0) for b0 in range(0, len(windows), B)]
        else:
            sizes = batch_sizes(len(windows), eng.max_batch, self.sub_batch_min)
        offs = np.cumsum([0] + sizes).tolist()
        parts = [windows[offs[k]: offs[k + 1]] for k in range(len(sizes))]
        on_device = torch.is_tensor(wav)
        on_gpu = on_device and wav.is_cuda
        if on_gpu and (wav.dtype != torch.float32 or not wav.is_contiguous()):
            wav = wav.to(torch.float32).contiguous()

        def load(k):  # called on the engine's encoder stream
            part = parts[k]
            if on_gpu:  # one launch gathers the batch's rows out of the waveform (the arena) in device memory
                n = len(part)
                start = (ctypes.c_int64 * n)(*[int(w.start) for w in part])
                length = (ctypes.c_int32 * n)(*[min(int(w.length), CHUNK_SAMPLES) for w in part])  # fe truncation
                _lib.call("tw_gather_windows", wav.data_ptr(), wav.numel(), start, length, n, CHUNK_SAMPLES,
                          eng.wave.data_ptr(), eng.wave.stride(0), torch.cuda.current_stream(wav.device).cuda_stream)
                return
            if on_device:  # a CPU tensor (gloo): slices of the rank's waveform copy
                dst = eng.wave[: len(part)]
                for j, w in enumerate(part):
                    n = min(w.length, CHUNK_SAMPLES)  # feature extractor truncation
                    dst[j, :n].copy_(wav[w.start: w.start + n], non_blocking=True)
                    dst[j, n:].zero_()
                return
            host = self._host_staging(k % 2, len(part))
            for j, w in enumerate(part):
                seg = wav[w.start: w.start + min(w.length, CHUNK_SAMPLES)]  # feature extractor truncation
                host[j, : len(seg)] = torch.from_numpy(np.ascontiguousarray(seg, np.float32))
                host[j, len(seg):] = 0
            eng.wave[: len(part)].copy_(host, non_blocking=host.is_pinned())
            if self._staging is not None:
                self._staging[1][k % 2].record(torch.cuda.current_stream(eng.wave.device))

        bkw = None
        if word_timestamps:
            bkw = [{"word_timestamps": True, "num_frames": list(num_frames[offs[k]: offs[k + 1]])}
                   for k in range(len(sizes))]
        res = eng.run_batches(sizes, load=load, batch_kwargs=bkw, task=task,
                              lang_ids=None if lang_id is None else [lang_id] * max(sizes, default=1),
                              max_new_tokens=max_new_tokens, return_timestamps=return_timestamps, num_beams=num_beams,
                              max_passes=max_passes,
                              **({"fallback": fallback, "window_offset": window_base} if fallback is not None else {}),
                              **({"condition_on_prev_tokens": True} if condition_on_prev_tokens else {}),
                              **(prompt or {}), **(history or {}),
                              **({"token_logprobs": True} if token_logprobs else {}),
                              **({"top_alternatives": int(top_alternatives)} if top_alternatives else {}))
        out: List[List[int]] = []
        for seqs in res:
            out.extend(pad_right(seqs, self.gen.special.eot))
        # per-window record of the last call (languages, raw tokens of every seek pass) for diagnostics/tests
        self.last_window_langs = [lg for bl in eng.batch_langs for lg in bl]
        self.last_window_passes = [p for bp in eng.batch_passes for p in bp]
        self.last_window_prefixes = [p for bp in eng.batch_prefixes for p in bp]
        if word_timestamps:  # per window the concatenated segments' token times (not padded, as the pipeline's)
            self.last_window_token_timestamps = [t for bt in eng.batch_token_timestamps for t in bt]
        if token_logprobs:
            self.last_window_pass_logprobs = [p for bp in eng.batch_pass_logprobs for p in bp]
            self.last_window_token_logprobs = [t for bt in eng.batch_token_logprobs for t in bt]
        if top_alternatives:
            self.last_window_token_alternatives = [t for bt in eng.batch_token_alternatives for t in bt]
        return out

    @staticmethod
    def _history_options(gk: Dict[str, Any], vocab: Optional[int] = None) -> Dict[str, Any]:
        """Pops generate()'s `repetition_penalty`, `no_repeat_ngram_size`, `length_penalty` and `sequence_bias`;
        returns those that are on as WhisperEngine.generate's kwargs (None, 1.0 and 0 mean off, as
        _get_logits_processor reads them). Values are checked as RepetitionPenaltyLogitsProcessor /
        NoRepeatNGramLogitsProcessor / SequenceBiasLogitsProcessor check them (generation/logits_process.py), with
        their messages. sequence_bias (a dict {tuple of ids: float} or a list of [ids, float]) comes back as a dict in
        the kernel's table order — 1-id entries first, then the rest, each in the dict's order; vocab: ids at or past
        it raise as transformers' first processor call does. `bad_words_ids` is left in place: the callable keeps
        refusing it as an unsupported kwarg (WhisperEngine.generate takes it; through the callable a sequence is
        forbidden with a sequence_bias of -inf, which yields the same scores: -inf survives the penalty and the
        n-gram stage unchanged)."""
        out: Dict[str, Any] = {}
        p = gk.pop("repetition_penalty", None)
        if p is not None and p != 1.0:
            if not isinstance(p, float) or not (p > 0):
                raise ValueError(f"`penalty` has to be a strictly positive float, but is {p}")
            out["repetition_penalty"] = p
        n = gk.pop("no_repeat_ngram_size", None)
        if n:  # (None and 0 are off, as generate() reads them)
            if not isinstance(n, int) or n <= 0:
                raise ValueError(f"`ngram_size` has to be a strictly positive integer, but is {n}")
            out["no_repeat_ngram_size"] = int(n)
        lp = gk.pop("length_penalty", None)
        if lp is not None and float(lp) != 1.0:
            out["length_penalty"] = float(lp)
        sb = gk.pop("sequence_bias", None)
        if sb is not None:
            pre = seqbias.sequence_bias_entries(sb, vocab)
            seqbias.check_limits(pre, [])
            out["sequence_bias"] = dict(pre)
        return out

    def _fallback_config(self, gk: Dict[str, Any]) -> FallbackConfig:
        """Pops generate()'s temperature-fallback kwargs (generation_whisper.py:398-401): `temperature` (a float or
        a list / tuple of temperatures tried in turn), the three segment criteria (else the checkpoint's
        generation_config values), `top_k` (sampling; GenerationConfig's default 50), `do_sample` (ignored: the
        temperature decides, as generate_with_fallback does), and the extension `seed` (the sampler's key).
        (condition_on_prev_tokens is popped by the caller.)"""
        g = self.gen
        t = gk.pop("temperature", None)
        temps = tuple(t) if isinstance(t, (list, tuple)) else (t,)
        gk.pop("do_sample", None)
        pick = lambda k: gk.pop(k) if gk.get(k) is not None else (gk.pop(k, None), getattr(g, k))[1]  # noqa: E731
        return FallbackConfig(temperatures=temps, compression_ratio_threshold=pick("compression_ratio_threshold"),
                              logprob_threshold=pick("logprob_threshold"), no_speech_threshold=pick("no_speech_threshold"),
                              top_k=int(gk.pop("top_k", 50) or 0), seed=int(gk.pop("seed", getattr(self, "sample_seed", 0))))

    def _host_staging(self, i: int, rows: int) -> torch.Tensor:
        """Pinned host buffer i (of two, alternating per batch) for a batch's waveforms: the upload is then an async
        copy on the encoder stream; a buffer is refilled only after its previous copy has completed."""
        wave = self.engine.wave
        if not (torch.is_tensor(wave) and wave.is_cuda):
            return torch.zeros(rows, CHUNK_SAMPLES, dtype=torch.float32)
        if self._staging is None:
            bufs = [torch.empty(wave.shape[0], CHUNK_SAMPLES, dtype=torch.float32, pin_memory=True) for _ in range(2)]
            self._staging = (bufs, [torch.cuda.Event() for _ in range(2)])
        self._staging[1][i].synchronize()
        return self._staging[0][i][:rows]


def batch_sizes(n: int, max_batch: int, sub_batch_min: Optional[int] = None) -> List[int]:
    """Engine batch sizes for n windows: ceil(n / max_batch) near-equal batches (e.g. 30 windows at 24 -> 15 + 15,
    so that the encoder of the second overlaps the decode of the first with the same work on each side), and two
    when a single batch would hold >= 2 * sub_batch_min windows."""
    if n <= 0:
        return []
    k = -(-n // max_batch)
    if k == 1 and sub_batch_min is not None and n >= 2 * sub_batch_min:
        k = 2
    base, rem = divmod(n, k)
    return [base + 1] * rem + [base] * (k - rem)


def _dims_from_checkpoint(path: str) -> WhisperDims:
    import json

    with open(os.path.join(path, "config.json")) as f:
        c = json.load(f)
    return WhisperDims(os.path.basename(os.path.normpath(path)), c["d_model"], c["encoder_layers"], c["decoder_layers"],
                       c["encoder_attention_heads"], c["encoder_ffn_dim"], c["num_mel_bins"], c["vocab_size"],
                       c.get("max_source_positions", 1500), c.get("max_target_positions", 448))
