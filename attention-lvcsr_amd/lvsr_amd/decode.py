"""Decode driver: what `lvsr.main.search` reports per utterance (lvsr/main.py:705-864) — beam search, negative
log-likelihood of the ground truth and of the best hypothesis through `analyze`, character/word error counts — around
`SpeechRecognizer.beam_search`.  Dataset access is the caller's business: utterances come in as
(recordings (T,F) ndarray, groundtruth label list) pairs."""
import numpy

from .error_rate import edit_distance, weights_std, monotonicity_penalty
from .search import CandidateNotFoundError


def _searched(recognizer, utterances, batch, kw):
    """(number, recordings, groundtruth, result of the beam search or the exception it raised), in order; `batch` > 1: the searches
    of that many utterances side by side in one set of launches (SpeechRecognizer.beam_search_batch)."""
    chunk = []
    for number, (recordings, groundtruth) in enumerate(utterances):
        if batch <= 1:
            try:
                yield number, recordings, groundtruth, recognizer.beam_search({"recordings": recordings}, **kw)
            except CandidateNotFoundError as e:
                yield number, recordings, groundtruth, e
            continue
        chunk.append((number, recordings, groundtruth))
        if len(chunk) == batch:
            for item, res in zip(chunk, recognizer.beam_search_batch([c[1] for c in chunk], **kw)):
                yield item + (res,)
            chunk = []
    if chunk:
        for item, res in zip(chunk, recognizer.beam_search_batch([c[1] for c in chunk], **kw)):
            yield item + (res,)


def _score_each(recognizer, recordings, groundtruth, recognized):
    """The two `analyze` calls of one utterance -> (groundtruth scores, scores of the hypothesis or None)."""
    inputs = {"recordings": recordings}
    gt_cost, gt_weights, _ = recognizer.analyze(inputs, numpy.asarray(groundtruth))
    gt = dict(cost=float(gt_cost.sum()), weights_std=float(weights_std(gt_weights[:, None, :])),
              monotonicity_penalty=float(monotonicity_penalty(gt_weights[:, None, :])))
    if not recognized:
        return gt, None
    rec_cost, _, _ = recognizer.analyze(inputs, numpy.asarray(groundtruth), numpy.asarray(recognized))
    return gt, dict(cost=float(rec_cost.sum()))


def _best(result):
    """the best hypothesis of a search result ([] where no candidate was found; None: no search was run)"""
    if result is None or isinstance(result, CandidateNotFoundError):
        return []
    if isinstance(result, Exception):
        raise result
    return result[0][0]


def _scored(recognizer, utterances, batch, kw, score_batch, nll_only):
    """(number, groundtruth, search result / exception / None under `nll_only`, groundtruth scores, hypothesis scores or None), in
    order.  `score_batch` = 0: utterance by utterance through `analyze`; N > 0: chunks of N utterances, each searched and then scored
    by ONE `analyze_batch` call."""
    if score_batch <= 0:
        items = ((n, x, g, None) for n, (x, g) in enumerate(utterances)) if nll_only else _searched(recognizer, utterances, batch, kw)
        for number, recordings, groundtruth, result in items:
            groundtruth = [int(t) for t in groundtruth]
            yield (number, groundtruth, result) + _score_each(recognizer, recordings, groundtruth, _best(result))
        return
    chunk = []

    def flush():
        results = [None] * len(chunk) if nll_only else [r for _, _, _, r in _searched(recognizer, [c[1:] for c in chunk], batch, kw)]
        scores = recognizer.analyze_batch([c[1] for c in chunk], [c[2] for c in chunk],
                                          None if nll_only else [_best(r) for r in results])
        for (number, _, groundtruth), result, sc in zip(chunk, results, scores):
            yield number, groundtruth, result, sc["groundtruth"], sc["prediction"]

    for number, (recordings, groundtruth) in enumerate(utterances):
        chunk.append((number, recordings, [int(t) for t in groundtruth]))
        if len(chunk) == score_batch:
            for item in flush():
                yield item
            chunk = []
    if chunk:
        for item in flush():
            yield item


def search(recognizer, utterances, beam_size=10, char_discount=0.0, round_to_inf=1e9, stop_on="patience", to_words=None,
           report=None, batch=1, score_batch=0, nll_only=False):
    """-> dict(per_utterance=[...], cer=, wer=, nll_groundtruth=, nll_recognized=).  `to_words(labels) -> list[str]` turns a
    label sequence into words for WER (the reference decodes characters with its character map, lvsr/main.py:788-800).
    `batch` (an addition): utterances decoded side by side, several times the throughput on a GPU.  An utterance's hypotheses do not
    depend on the batch it is decoded in for any batch > 1 (trailing chunks and one-utterance chunks included: the readout's merge
    products always run through lvsr_readout_merge there); against batch = 1 (per-row VALU products below 64 rows: another float32
    summation order) costs agree to ~1e-5 relative and candidates closer than that may swap ranks.  A host-side language model
    or a validator decode one utterance at a time whatever `batch` says (BeamSearch.search_batch).
    `score_batch` (an addition): 0 = every utterance is scored by two `analyze` calls at batch 1, its alignment reduced on the host;
    N > 0 = utterances are taken in chunks of N, a chunk is searched (side by side with `batch` > 1) and then scored by one
    `SpeechRecognizer.analyze_batch` call: one encoder pass, two ragged decoder passes, the report's reductions on the device.  The
    rows carry the same keys either way and `report(row)` is called in utterance order.
    `nll_only` (the reference's --nll-only, lvsr/main.py:793-795): no search; the rows hold the ground-truth scores only and the
    result has no cer / wer / nll_recognized.
    nll_groundtruth: the mean ground-truth cost per utterance (the reference's "Average groundtruth cost"); nll_recognized: the mean
    cost of the best hypothesis over the utterances that have one (nan when none has)."""
    if not nll_only:
        recognizer.init_beam_search(beam_size)
    rows, tot_err, tot_len, tot_werr, tot_wlen = [], 0, 0, 0, 0
    tot_gt, tot_rec, num_rec = 0.0, 0.0, 0
    kw = dict(char_discount=char_discount, round_to_inf=round_to_inf, stop_on=stop_on)
    for number, groundtruth, result, gt, rec in _scored(recognizer, utterances, int(batch), kw, int(score_batch), bool(nll_only)):
        row = dict(number=number, groundtruth=groundtruth)
        recognized = _best(result)
        if isinstance(result, CandidateNotFoundError):                       # lvsr/main.py:808-813
            row.update(recognized=[], search_cost=float("nan"), error="CandidateNotFoundError")
        elif result is not None:
            row.update(recognized=recognized, search_cost=result[1][0])
        row.update(groundtruth_cost=gt["cost"], weights_std=gt["weights_std"], monotonicity_penalty=gt["monotonicity_penalty"])
        tot_gt += gt["cost"]
        if rec is not None:
            row["recognized_cost"] = rec["cost"]
            tot_rec += rec["cost"]
            num_rec += 1
        if not nll_only:
            err = int(edit_distance(groundtruth, recognized))
            row.update(char_errors=err, cer=err / float(len(groundtruth)))
            tot_err += err
            tot_len += len(groundtruth)
            if to_words is not None:
                gw, rw = to_words(groundtruth), to_words(recognized)
                werr = int(edit_distance(gw, rw))
                row.update(word_errors=werr, wer=werr / float(max(1, len(gw))))
                tot_werr += werr
                tot_wlen += len(gw)
        rows.append(row)
        if report is not None:
            report(row)
    out = dict(per_utterance=rows, nll_groundtruth=tot_gt / float(max(1, len(rows))))
    if nll_only:
        return out
    out.update(cer=tot_err / float(max(1, tot_len)), nll_recognized=tot_rec / num_rec if num_rec else float("nan"))
    if to_words is not None:
        out["wer"] = tot_werr / float(max(1, tot_wlen))
    return out


def recognize_plan(num_samples, batch, sort=True):
    """The chunks `recognize` decodes: lists of indices into `num_samples` (the utterances' sample counts).  sort=True: in order of
    decreasing length (equal lengths in input order), cut into chunks of `batch` — the utterances of a chunk are padded to its
    longest, so chunks of like lengths mean less padding and fewer distinct graph shapes; sort=False: input order."""
    batch = max(1, int(batch))
    order = list(range(len(num_samples)))
    if sort:
        order.sort(key=lambda i: (-int(num_samples[i]), i))
    return [order[i: i + batch] for i in range(0, len(order), batch)]


def token_times(rows, labels, subsample, frame_shift, frame_length, sample_rate, num_frames, mse=False):
    """Alignment rows to seconds (pure host arithmetic): `rows` (L,8) as `SpeechRecognizer.align_batch` returns them for one
    utterance, `labels` its L labels, `subsample` the encoder's per-layer factors, `frame_shift` / `frame_length` in samples,
    `num_frames` the utterance's frames -> a list of dict(label=, start=, end=, peak=, confidence=), times in seconds.
    With S = prod(subsample): the reference's encoder takes [::k] behind every layer (lvsr/bricks/__init__.py:75-77), so attended position p
    stands for the input frames from p S on, and
      start = start_pos S shift,   end = min((end_pos + 1) S shift, duration),   peak = the middle of the span of peak_pos,
    all clipped to duration = ((num_frames - 1) frame_shift + frame_length) / sample_rate.  The times are NOMINAL: the contexts come
    out of a bidirectional network that has seen the whole utterance, so a position covers its S frames only by construction.
    confidence = exp(-cost), the probability the model gave the label (with a language model attached: the fused one).  `mse`: under
    an mse criterion the cost is a squared error, not a log-probability, so the key is left out."""
    rows = numpy.asarray(rows, numpy.float64).reshape(-1, 8)
    if len(rows) != len(labels):
        raise ValueError("token_times: %d rows for %d labels" % (len(rows), len(labels)))
    span = float(numpy.prod([int(k) for k in subsample])) * float(frame_shift) / float(sample_rate)
    duration = ((int(num_frames) - 1) * float(frame_shift) + float(frame_length)) / float(sample_rate)
    out = []
    for label, r in zip(labels, rows):
        token = dict(label=int(label), start=min(float(r[4]) * span, duration), end=min((float(r[5]) + 1.0) * span, duration),
                     peak=min((float(r[0]) + 0.5) * span, duration))
        if not mse:
            token["confidence"] = float(numpy.exp(-r[7]))
        out.append(token)
    return out


def group_words(tokens, word_boundary):
    """Tokens of `token_times` to words: `word_boundary` is a set of labels (space, EOS, ...); a word is a run of tokens that are
    not in it -> a list of dict(labels=, start=, end=, confidence=): start of its first token, end of its last, the smallest token
    confidence (absent when the tokens carry none).  Boundary tokens belong to no word."""
    boundary = set(int(b) for b in word_boundary)
    words, run = [], []

    def close():
        if run:
            word = dict(labels=[t["label"] for t in run], start=run[0]["start"], end=run[-1]["end"])
            if all("confidence" in t for t in run):
                word["confidence"] = min(t["confidence"] for t in run)
            words.append(word)
            del run[:]
    for t in tokens:
        if t["label"] in boundary:
            close()
        else:
            run.append(t)
    close()
    return words


def _waveform_items(recognizer, front_end, waveforms, where):
    """[(id, samples)], their sample counts — behind the refusals `recognize` and `align` share"""
    items = []
    for number, w in enumerate(waveforms):
        ident, samples = w if isinstance(w, tuple) else (number, w)
        items.append((ident, samples))
    if front_end.num_features != recognizer.d.F:
        raise ValueError("%s: the front end makes %d features per frame, the recognizer takes %d" % (where, front_end.num_features, recognizer.d.F))
    num_samples = [int(len(s)) for _, s in items]
    for (ident, _), n in zip(items, num_samples):
        if front_end.num_frames(n) <= 0:
            raise ValueError("%s: utterance %r has %d samples, fewer than one frame (%d samples)" % (where, ident, n, front_end.fbank.frame_length))
    return items, num_samples


def _timed(recognizer, front_end, row, rows8, labels, word_boundary):
    """adds tokens= (and words=) to `row` from the alignment rows of its labels"""
    fb = front_end.fbank
    row["tokens"] = token_times(rows8, labels, recognizer.d.subsample, fb.frame_shift, fb.frame_length, front_end.sample_rate,
                                row["num_frames"], mse=recognizer.generator.mse)
    if word_boundary is not None:
        row["words"] = group_words(row["tokens"], word_boundary)


def recognize(recognizer, front_end, waveforms, beam_size=10, batch=64, char_discount=0.0, round_to_inf=1e9, stop_on="patience",
              to_text=None, sort=True, timestamps=False, quantiles=(0.1, 0.9), word_boundary=None):
    """From waveforms to hypotheses: `waveforms` is a sequence of 1-D int16 arrays or of (id, array) pairs (ids default to the
    position); `front_end` a `frontend.FrontEnd`.  Each chunk of `recognize_plan` goes through FrontEnd.batch (two launches; the PCM
    is all that is copied to the device) and SpeechRecognizer.beam_search_staged.  -> one row per utterance IN INPUT ORDER:
    dict(id=, recognized=, search_cost=, num_frames=) and text= when `to_text(labels)` is given; an utterance whose search finds no
    candidate has recognized=[], search_cost=nan and error="CandidateNotFoundError", as in `search`.
    `timestamps` (an addition): every row also carries tokens= (`token_times` of its recognised labels; [] where no candidate was
    found) and, with `word_boundary` (a set of labels), words= (`group_words`).  Behind a chunk's search its best hypotheses are
    aligned by one `SpeechRecognizer.align_staged` call that teacher-forces over the contexts the search was started from — no second
    encoder pass —, one lvsr_alignment_times launch and one small copy per chunk; `quantiles` are the shares of a label's alignment
    mass at which it starts and ends.  Without `timestamps` the launches and the rows are what they were."""
    items, num_samples = _waveform_items(recognizer, front_end, waveforms, "recognize")
    recognizer.init_beam_search(beam_size)
    kw = dict(char_discount=char_discount, round_to_inf=round_to_inf, stop_on=stop_on)
    rows = [None] * len(items)
    for chunk in recognize_plan(num_samples, batch, sort):
        x, mask, lengths = front_end.batch([items[i][1] for i in chunk])
        for i, n, result in zip(chunk, lengths, recognizer.beam_search_staged(x, mask, lengths, **kw)):
            row = dict(id=items[i][0], num_frames=int(n))
            if isinstance(result, CandidateNotFoundError):
                row.update(recognized=[], search_cost=float("nan"), error="CandidateNotFoundError")
            elif isinstance(result, Exception):
                raise result
            else:
                row.update(recognized=result[0][0], search_cost=result[1][0])
            if to_text is not None:
                row["text"] = to_text(row["recognized"])
            rows[i] = row
        if timestamps:
            best = [rows[i]["recognized"] for i in chunk]
            for i, rows8 in zip(chunk, recognizer.align_staged(x, mask, lengths, best, quantiles=quantiles, reuse_contexts=True)):
                _timed(recognizer, front_end, rows[i], rows8, rows[i]["recognized"], word_boundary)
    return rows


def align(recognizer, front_end, waveforms, transcripts, batch=64, quantiles=(0.1, 0.9), word_boundary=None, sort=True):
    """Forced alignment: when was each label of a GIVEN label sequence said.  `waveforms` as for `recognize`, `transcripts` one label
    sequence per waveform (as the recognizer was trained on them: with EOS where the data had it).  Chunks of `recognize_plan`, each
    through FrontEnd.batch and one `SpeechRecognizer.align_staged` call (one encoder pass, one teacher-forced pass, one
    lvsr_alignment_times launch, one small copy).  -> one row per utterance IN INPUT ORDER: dict(id=, num_frames=, cost= the summed
    cost of the labels, tokens=) and words= when `word_boundary` is given (`token_times`, `group_words`).  The refusals of `recognize`
    — another feature width, an utterance shorter than one frame —, and a `transcripts` of another length than `waveforms`."""
    waveforms = list(waveforms)
    transcripts = [[int(t) for t in s] for s in transcripts]
    if len(transcripts) != len(waveforms):
        raise ValueError("align: %d waveforms, %d transcripts" % (len(waveforms), len(transcripts)))
    items, num_samples = _waveform_items(recognizer, front_end, waveforms, "align")
    rows = [None] * len(items)
    for chunk in recognize_plan(num_samples, batch, sort):
        x, mask, lengths = front_end.batch([items[i][1] for i in chunk])
        aligned = recognizer.align_staged(x, mask, lengths, [transcripts[i] for i in chunk], quantiles=quantiles)
        for i, n, rows8 in zip(chunk, lengths, aligned):
            rows[i] = dict(id=items[i][0], num_frames=int(n), cost=float(rows8[:, 7].sum()))
            _timed(recognizer, front_end, rows[i], rows8, transcripts[i], word_boundary)
    return rows
