"""Evaluation-time sentence selection (reference: Tester.py:8-196, tools/utils.py:45-55).

Same classes, constructor arguments, ``evaluation(G, index, dataset, blocking)``
contract and accumulated state (``extracts``, ``hyps``, ``refer``, ``running_avg_loss``,
``pred/true/match/match_true``, ``getMetric`` -> accu / precision / recall / F) as the
reference, so evaluation.py's loop and ``train.py``'s validation run unchanged.

What differs is *how*: the reference unbatches the graph and, per document, filters
its sentence nodes, runs ``topk`` and compares against the labels (Tester.py:105-140)
-- a Python loop of small tensor ops per document.  Here the per-document loss sums,
the top-k selection (one ``topk`` over the [docs, max_sentences] padded score
matrix) and the match counters are batched tensor ops on the logits' device, with
one device->host copy per batch for the selected indices; only the string work
(n-gram blocking, hypothesis assembly) stays on the host.

Opt-in (``path_options(HSG_EVAL_SELECT="1")``): the native evaluation step.  The loss is
``hsg_doc_ce``, the selection -- n-gram blocking included -- and the match counters are one
``hsg_eval_select`` launch (evalsel.py, include/hsg_eval.h), the loss sum and the counters
stay in device accumulators, and the selected indices come back through pinned buffers
behind an event, so that the host's string work for batch i-1 overlaps the device's work
for batch i.  ``SLTester.sync()`` drains everything; the accessors call it, direct reads
of the plain attributes (``extracts``, ``pred``, ``running_loss``...) need it first.  The
order among EQUAL scores in that mode is include/hsg_eval.h's (ascending index), not
torch's.

``path_options(HSG_EVAL_SELECT="words")`` is the same step with another blocking operand:
the device takes each sentence's document-local word ids and forms the n-gram windows itself
(``hsg_eval_select_words``, include/hsg_eval_words.h), so the host does no n-gram work.  The
ids come from the graph when the dataset attached them in its workers
(``ExampleSet(eval_words=True)`` -> ``G.eval_words``), else from ``evalsel.words_for``'s
per-example cache.

``path_options(HSG_EVAL_SELECT="text")`` is that step with the word ids made on the device: the
host encodes the article sentences and hands over their bytes (``evalsel.pack_text``), the
device splits them at ``str.split()``'s whitespace and interns the words
(``hsg_eval_text_words``, include/hsg_eval_text.h), and the unchanged ``hsg_eval_select_words``
selects.  Ids attached to the graph are used as they are; the per-example cache is neither
read nor filled.

In both of these modes a resident batch that carries the eval view (``G.eval_pack``,
``resident.DocumentStore.batch``, include/hsg_resident_eval.h) brings its word pack along, already
on the device: nothing is packed, pinned or uploaded here, the seen set is sized from the
store's cache, and the batch's examples are read from the dataset in ``_drain``, behind the
launches.
"""
from __future__ import annotations

import datetime
import logging
import os

import torch

from . import _lib
from .HiGraph import node_ids, sentence_counts

logger = logging.getLogger("Summarization logger")


def eval_label(match_true, pred, true, total, match):
    """tools/utils.py:45-55 (tensor arithmetic: a zero count gives nan/inf, as there)."""
    match_true, pred, true, match = (torch.as_tensor(x).float() for x in (match_true, pred, true, match))
    try:
        accu = match / total
        precision = match_true / pred
        recall = match_true / true
        F = 2 * precision * recall / (precision + recall)
    except ZeroDivisionError:
        accu, precision, recall, F = 0.0, 0.0, 0.0, 0.0
        logger.error("[Error] float division by zero")
    return accu, precision, recall, F


class TestPipLine:
    """Tester.py:8-75."""

    def __init__(self, model, m, test_dir, limited):
        self.model = model
        self.limited = limited
        self.m = m
        self.test_dir = test_dir
        self.extracts = []
        self.batch_number = 0
        self.running_loss = 0
        self.example_num = 0
        self.total_sentence_num = 0
        self._hyps = []
        self._refer = []

    def evaluation(self, G, index, valset):
        pass

    def getMetric(self):  # noqa: N802 (reference name)
        pass

    def SaveDecodeFile(self):  # noqa: N802
        now = datetime.datetime.now().strftime("%Y%m%d_%H%M%S")
        with open(os.path.join(self.test_dir, now), "wb") as f:
            for i in range(self.rougePairNum):
                f.write(b"[Reference]\t" + self._refer[i].encode("utf-8") + b"\n")
                f.write(b"[Hypothesis]\t" + self._hyps[i].encode("utf-8") + b"\n\n\n")

    @property
    def running_avg_loss(self):
        return self.running_loss / self.batch_number

    @property
    def rougePairNum(self):  # noqa: N802
        return len(self._hyps)

    @property
    def hyps(self):
        if not self.limited:
            return self._hyps
        # limited-length recall: cut each hypothesis to its reference's word count
        return [" ".join(h.split(" ")[:len(r.split(" "))]) for h, r in zip(self._hyps, self._refer)]

    @property
    def refer(self):
        return self._refer

    @property
    def extractLabel(self):  # noqa: N802
        return self.extracts


def _select(p_sent, counts, m):
    """Per-document selected sentence indices (local), in the reference's order:
    m == 0 -> argmax(p) != 0 in ascending index order (Tester.py:115-117); else
    topk(p[:, 1], min(m, N)) in descending score order (124)."""
    dev = p_sent.device
    B = len(counts)
    if m == 0:
        pred = p_sent.max(1)[1].ne(0).cpu()
        out, o = [], 0
        for n in counts:
            out.append(torch.nonzero(pred[o:o + n]).view(-1))
            o += n
        return out
    nmax = max(counts) if counts else 0
    cnt = torch.tensor(counts, device=dev)
    seg = torch.repeat_interleave(torch.arange(B, device=dev), cnt)
    start = torch.cumsum(cnt, 0) - cnt
    local = torch.arange(p_sent.shape[0], device=dev) - start[seg]
    score = p_sent.new_full((B, max(nmax, 1)), float("-inf"))
    score[seg, local] = p_sent[:, 1]
    k = min(m, nmax)
    top = torch.topk(score, k, dim=1).indices.cpu() if k > 0 else torch.zeros(B, 0, dtype=torch.long)
    return [top[j, :min(m, n)] for j, n in enumerate(counts)]


class SLTester(TestPipLine):
    """Tester.py:78-196."""

    def __init__(self, model, m, test_dir=None, limited=False, blocking_win=3):
        super().__init__(model, m, test_dir, limited)
        self.pred, self.true, self.match, self.match_true = 0, 0, 0, 0
        self._F = 0
        self.criterion = torch.nn.CrossEntropyLoss(reduction="none")
        self.blocking_win = blocking_win
        self._pending = None                 # native path: the batch whose indices are in flight
        self._acc = None                     # native path: device accumulators (totals int64 [4], loss fp64)
        self._acc_dirty = False

    def evaluation(self, G, index, dataset, blocking=False):
        mode = _lib.path_option("HSG_EVAL_SELECT", "0")
        if mode in ("1", "words", "text"):
            return self._evaluation_native(G, index, dataset, blocking, mode)
        self.batch_number += 1
        outputs = self.model.forward(G)
        snode = node_ids(G, "dtype", 1.0)
        label = G.ndata["label"][snode].sum(-1)                               # [n_sent]
        counts = sentence_counts(G)
        B = len(counts)
        # dgl.sum_nodes(G, "loss").mean(): per-document sums of the sentence losses
        seg = torch.repeat_interleave(torch.arange(B, device=outputs.device),
                                      torch.tensor(counts, device=outputs.device))
        loss_s = self.criterion(outputs, label)
        per_doc = loss_s.new_zeros(B).index_add(0, seg, loss_s)
        self.running_loss += float(per_doc.mean())

        p_host = outputs.detach().cpu() if blocking else None
        sel = None if blocking else _select(outputs.detach(), counts, self.m)
        label_h = label.cpu()
        o = 0
        for j in range(B):
            N = counts[j]
            example = dataset.get_example(index[j])
            sents = example.original_article_sents
            if blocking and self.m != 0:
                pred_idx = self.ngram_blocking(sents, p_host[o:o + N, 1], self.blocking_win, min(self.m, N))
            elif blocking:
                pred_idx = _select(p_host[o:o + N], [N], 0)[0]
            else:
                pred_idx = sel[j]
            prediction = torch.zeros(N, dtype=torch.long)
            prediction[pred_idx] = 1
            lab = label_h[o:o + N]
            self.extracts.append(pred_idx.tolist())
            self.pred += prediction.sum()
            self.true += lab.sum()
            self.match_true += ((prediction == lab) & (prediction == 1)).sum()
            self.match += (prediction == lab).sum()
            self.total_sentence_num += N
            self.example_num += 1
            self._hyps.append("\n".join(sents[i] for i in pred_idx.tolist() if i < len(sents)))
            self._refer.append(example.original_abstract)
            o += N

    # ---- the native evaluation step (HSG_EVAL_SELECT=1, =words or =text) -------------------
    def _evaluation_native(self, G, index, dataset, blocking, mode="1"):
        from . import evalsel, loss
        self.batch_number += 1
        outputs = self.model.forward(G)
        if not (torch.is_tensor(outputs) and outputs.is_cuda and outputs.dtype == torch.float32):
            raise RuntimeError(f"SLTester (HSG_EVAL_SELECT={mode}): the model's logits must be fp32 on a ROCm device "
                               "(no fallback)")
        outputs = outputs.detach()
        dev = outputs.device
        counts = sentence_counts(G)
        B = len(counts)
        # a resident batch with the eval view carries its word pack, assembled on the device
        # (resident.DocumentStore.batch, G.eval_pack): nothing is packed or uploaded here, and
        # the dataset is first read in _drain, behind the launches
        view = getattr(G, "eval_pack", None) if blocking and self.m != 0 and mode in ("words", "text") else None
        # host work while the forward runs: the examples and the blocking operands
        examples = None if view is not None else [dataset.get_example(index[j]) for j in range(B)]
        pack = text = None
        if view is not None:
            pack = view
        elif blocking and self.m != 0 and mode in ("words", "text"):
            # word ids: from the graph if the dataset attached them; else made once per example
            # ("words"), or made on the device from the sentences' bytes ("text")
            parts = getattr(G, "eval_words", None)
            if parts is None and mode == "text":
                text = evalsel.pack_text([e.original_article_sents for e in examples], counts)
            else:
                if parts is None:
                    parts = [evalsel.words_for(dataset, index[j], examples[j].original_article_sents, counts[j])
                             for j in range(B)]
                pack = evalsel.pack_words(parts, counts)
        elif blocking and self.m != 0:
            pack = evalsel.pack_batch([e.original_article_sents for e in examples], counts, self.blocking_win)
        rows, labels, doc_off = loss.sentence_loss_inputs(G)
        mean = loss.doc_cross_entropy(outputs, labels, doc_off, rows)[0]
        if self._acc is None or self._acc[0].device != dev:
            self.sync()
            self._acc = (torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros((), dtype=torch.float64, device=dev))
        totals, loss_sum = self._acc
        loss_sum.add_(mean)
        label = labels[rows].sum(-1)                                          # [n_sent]
        n_max = max(max(counts), 1)
        sel_ld = n_max if self.m == 0 else min(self.m, n_max)
        out = torch.empty(B * (sel_ld + 1 + 4), dtype=torch.int32, device=dev)
        views = (out[:B * sel_ld].view(B, sel_ld), out[B * sel_ld:B * (sel_ld + 1)], out[B * (sel_ld + 1):].view(B, 4))
        if text is not None:
            evalsel.select_words(outputs, label, doc_off, self.m, n_max, self.blocking_win, totals,
                                 evalsel.text_words(text.to(dev), doc_off), text.tab_cap(self.blocking_win, self.m),
                                 sel_ld, views)
        elif mode in ("words", "text"):
            evalsel.select_words(outputs, label, doc_off, self.m, n_max, self.blocking_win, totals,
                                 None if pack is None else pack.to(dev), None, sel_ld, views)
        else:
            evalsel.select(outputs, label, doc_off, self.m, n_max, totals, None if pack is None else pack.to(dev),
                           sel_ld, views)
        self._acc_dirty = True
        host = torch.empty(B * (sel_ld + 1), dtype=torch.int32, pin_memory=True)
        host.copy_(out[:B * (sel_ld + 1)], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        source = None if examples is not None else (dataset, [index[j] for j in range(B)])
        prev, self._pending = self._pending, (ev, host, sel_ld, counts, examples, mode, source)
        if prev is not None:
            self._drain(prev)

    def _drain(self, pending):
        """The host half of one batch (Tester.py:138-143), once its indices have arrived."""
        ev, host, sel_ld, counts, examples, mode, source = pending
        if examples is None:                 # an eval-view batch: its examples are read here
            examples = [source[0].get_example(i) for i in source[1]]
        ev.synchronize()
        B = len(counts)
        sel = host[:B * sel_ld].view(B, sel_ld).tolist()
        nsel = host[B * sel_ld:].tolist()
        for j in range(B):
            if nsel[j] < 0 and mode in ("words", "text"):
                raise RuntimeError(f"SLTester (HSG_EVAL_SELECT={mode}): document {j} of the batch is beyond "
                                   "hsg_eval_select_words's limits (its rows, or the windows of its chosen sentences)")
            if nsel[j] < 0:
                raise RuntimeError(f"SLTester (HSG_EVAL_SELECT=1): document {j} of the batch is beyond hsg_eval_select's "
                                   "limits or carries an invalid n-gram id")
            pred_idx = sel[j][:nsel[j]]
            sents = examples[j].original_article_sents
            self.extracts.append(pred_idx)
            self.total_sentence_num += counts[j]
            self.example_num += 1
            self._hyps.append("\n".join(sents[i] for i in pred_idx if i < len(sents)))
            self._refer.append(examples[j].original_abstract)

    def sync(self):
        """Native path: drain the batch in flight and move the device accumulators into
        ``pred / true / match_true / match`` and ``running_loss`` (one read-back).  A no-op
        when nothing is outstanding."""
        prev, self._pending = self._pending, None
        if prev is not None:
            self._drain(prev)
        if self._acc_dirty:
            totals, loss_sum = self._acc
            t = totals.tolist()
            self.running_loss += float(loss_sum)
            totals.zero_()
            loss_sum.zero_()
            self._acc_dirty = False
            self.pred += torch.tensor(t[0])
            self.true += torch.tensor(t[1])
            self.match_true += torch.tensor(t[2])
            self.match += torch.tensor(t[3])

    @property
    def running_avg_loss(self):
        self.sync()
        return self.running_loss / self.batch_number

    @property
    def rougePairNum(self):  # noqa: N802
        self.sync()
        return len(self._hyps)

    @property
    def hyps(self):
        self.sync()
        return TestPipLine.hyps.fget(self)

    @property
    def refer(self):
        self.sync()
        return self._refer

    @property
    def extractLabel(self):  # noqa: N802
        self.sync()
        return self.extracts

    def SaveDecodeFile(self):  # noqa: N802
        self.sync()
        super().SaveDecodeFile()

    def getMetric(self):  # noqa: N802
        self.sync()
        logger.info("[INFO] Validset match_true %d, pred %d, true %d, total %d, match %d",
                    self.match_true, self.pred, self.true, self.total_sentence_num, self.match)
        self._accu, self._precision, self._recall, self._F = eval_label(
            self.match_true, self.pred, self.true, self.total_sentence_num, self.match)
        logger.info("[INFO] The size of totalset is %d, sent_number is %d, accu is %f, precision is %f, "
                    "recall is %f, F is %f", self.example_num, self.total_sentence_num, self._accu,
                    self._precision, self._recall, self._F)

    def ngram_blocking(self, sents, p_sent, n_win, k):
        """Tester.py:161-191: greedy by descending score, skip a sentence sharing an
        n-gram with the ones already chosen.  Keeps the reference's window range
        ``range(len(pieces) - n_win)`` (the last n-gram of a sentence is not used)."""
        seen = set()
        chosen = []
        for idx in p_sent.sort(descending=True)[1].tolist():
            pieces = sents[idx].split()
            grams = [" ".join(pieces[i:i + n_win]) for i in range(len(pieces) - n_win)]
            if any(g in seen for g in grams):
                continue
            chosen.append(idx)
            seen.update(grams)
            if len(chosen) >= k:
                break
        return torch.LongTensor(chosen)

    @property
    def labelMetric(self):  # noqa: N802
        return self._F
