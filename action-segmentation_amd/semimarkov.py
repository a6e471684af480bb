"""``SemiMarkovModel``: host harness of ``--classifier semimarkov`` (reference ``src/models/semimarkov/semimarkov.py``).

Same class surface as the reference (``add_args`` :17, ``from_args`` :34, ``fit_supervised`` :125,
``make_additional_allowed_ends`` :135, ``expand_constraints`` :149, ``fit`` :159, ``predict`` :318; attributes
``.model`` / ``.args``) so ``main.py``'s ``CLASSIFIERS['semimarkov']`` can point here unchanged.  ``predict``
returns ``{video_name: np.ndarray[int64, T]}`` of global class ids, no EOS id.

What is different is the batching of the decode: the reference calls ``viterbi`` once per single-task batch of
``--batch_size`` videos; here all those batches are folded into ONE ragged launch (batching.pack_batches), which is
what lets 256 CUs work on a corpus.  ``predict(test_data, fused=False)`` keeps the reference's call pattern.
"""
import numpy as np
import torch

from . import semimarkov_utils
from .batching import make_data_loader, make_optimizer, pack_batches
from .semimarkov_modules import SemiMarkovModule, all_equal


class SemiMarkovModel(object):
    DECODE_DEPTH = 8      # predict(fused=False): single-task batches in flight, one pinned result slot each ...
    STREAM_MIN_FRAMES = 1500   # ... and a stream each when the batch's longest video is at least this long: below, the GPU is
                               # done with a batch (0.17 us per frame) before the host has launched the next (0.25 ms), and
                               # a second stream would only add its hand-over (refdef, T <= 600: 4.4 -> 5.1 ms for 18 batches)

    DECODERS = ('viterbi', 'mbr')

    @classmethod
    def add_args(cls, parser):
        SemiMarkovModule.add_args(parser)
        # which segmentation predict() returns: the most probable one, or the one with the most expected correct frames
        # (minimum-Bayes-risk decode under frame loss, the metric evaluation reports)
        parser.add_argument('--sm_decoder', choices=list(cls.DECODERS), default='viterbi')
        parser.add_argument('--sm_component_model', action='store_true')
        parser.add_argument('--sm_constrain_transitions', action='store_true')
        parser.add_argument('--sm_constrain_with_narration', choices=['train', 'test'], nargs='*', default=[])
        parser.add_argument('--sm_constrain_narration_weight', type=float, default=-1e4)
        parser.add_argument('--sm_train_discriminatively', action='store_true')
        parser.add_argument('--sm_hidden_markov', action='store_true',
                            help='train as hidden markov model (fix K=1) and length distribution')
        parser.add_argument('--sm_predict_single', action='store_true')

    @classmethod
    def from_args(cls, args, train_data):
        n_classes = train_data.corpus.n_classes
        feature_dim = train_data.feature_dim
        allow_self_transitions = True
        assert args.sm_max_span_length is not None
        if getattr(args, 'sm_component_model', False):
            raise NotImplementedError("--sm_component_model (compound model) is outside the decode path built here")
        if args.sm_constrain_transitions:
            (allowed_starts, allowed_transitions, allowed_ends,
             ordered_indices_by_task) = train_data.get_allowed_starts_and_transitions()
            for src in range(n_classes):
                allowed_transitions.setdefault(src, set()).add(src)
        else:
            allowed_starts = allowed_transitions = allowed_ends = ordered_indices_by_task = None
        merge_classes = None
        if getattr(args, 'annotate_background_with_previous', False) and not getattr(args, 'no_merge_classes', False):
            merge_classes = {}
            bkg = set(train_data.corpus._background_indices)
            for task, indices in train_data.corpus._indices_by_task.items():
                background = [ix for ix in indices if ix in bkg]
                canon = background[0]
                for ix in indices:
                    tgt = canon if ix in bkg else ix
                    assert merge_classes.setdefault(ix, tgt) == tgt
        model = SemiMarkovModule(args, n_classes, feature_dim, allow_self_transitions=allow_self_transitions,
                                 allowed_starts=allowed_starts, allowed_transitions=allowed_transitions,
                                 allowed_ends=allowed_ends, merge_classes=merge_classes)
        return SemiMarkovModel(args, n_classes, feature_dim, model, ordered_indices_by_task)

    def __init__(self, args, n_classes, feature_dim, model, ordered_indices_by_task=None):
        self.args = args
        self.n_classes = n_classes
        self.feature_dim = feature_dim
        self.model = model
        self.ordered_indices_by_task = ordered_indices_by_task
        if args.cuda:
            self.model.cuda()

    @property
    def device(self):
        return self.model.gaussian_means.device

    # ------------------------------------------------------------------ training
    def fit_supervised(self, train_data):
        assert not self.args.sm_constrain_transitions
        loader = make_data_loader(self.args, train_data, batch_by_task=False, shuffle=False, batch_size=1)
        features, labels = [], []
        for batch in loader:
            features.append(batch['features'].squeeze(0))
            labels.append(batch['gt_single'].squeeze(0))
        self.model.fit_supervised(features, labels)

    def fit(self, train_data, use_labels, callback_fn=None):
        """reference semimarkov.py:159-316: closed form for supervised data, otherwise Adam on -log-likelihood
        (marginal likelihood log Z for unlabelled data; joint or conditional span score for labelled data)."""
        import time
        args = self.args
        self.model.train()
        if use_labels:
            assert not args.sm_constrain_transitions
        initialize = True
        if use_labels and args.sm_supervised_method in ('closed-form', 'closed-then-gradient'):
            self.fit_supervised(train_data)
            if args.sm_supervised_method == 'closed-then-gradient':
                initialize = False
                if callback_fn:
                    callback_fn(-1, {})
            else:
                return   # closed form: no epochs, callback never called (reference :165-171)
        optimizer, scheduler = make_optimizer(args, [p for p in self.model.parameters() if p.requires_grad])
        if initialize:
            big = next(iter(make_data_loader(args, train_data, batch_by_task=False, shuffle=True, batch_size=100)))
            self.model.initialize_gaussian(big['features'].to(self.device), big['lengths'])
        loader = make_data_loader(args, train_data, batch_by_task=True, shuffle=True, batch_size=args.batch_size)
        k = args.sm_max_span_length
        # Unlabelled data with --batch_accumulation > 1: the batches of one optimiser step go through ONE launch of each
        # kernel (log_likelihood_packed) instead of one latency-bound launch pair per batch of 5 videos; the loss is the
        # same mean over batches of the batch-mean -log Z, so the step is the reference's step.
        packed = (not use_labels) and args.batch_accumulation > 1
        train_cons = self._train_constraints(train_data)
        # Data-parallel training under torch.distributed: every rank walks the same shuffled batch order
        # (the sampler's RNG is seeded identically), the batches of one optimiser step are dealt round-robin to the
        # ranks, each rank back-propagates the sum of its batches' losses / --batch_accumulation, and ONE all-reduce
        # sums the gradients of every trained parameter (the five table tensors, and the flow's under --sm_feature_projection):
        # the step is the single-process step.  (One batch per step,
        # --batch_accumulation 1, cannot be split: the ranks then repeat the batch and average, which keeps their
        # parameters bit-identical although the kernels' atomics round differently from run to run.)
        from . import distributed
        dp = distributed.active()
        if dp:
            import torch.distributed as dist
            rank, world = dist.get_rank(), dist.get_world_size()
            distributed.broadcast_parameters(self.model)
        trained = [p for p in self.model.parameters() if p.requires_grad]
        for epoch in range(args.epochs):
            start_time = time.time()
            self.model.train()
            losses, pending = [], []
            train_nll = num_frames = num_videos = 0

            def step(batch_ix):
                if args.print_every and batch_ix % args.print_every == 0 and (not dp or rank == 0):
                    print('Epoch: %02d, Batch: %03d/%03d, loss: %.4f, recon: %.4f, Throughput: %.2f vid / sec' % (
                        epoch, batch_ix, len(loader), train_nll / num_videos, train_nll / num_frames,
                        num_videos / (time.time() - start_time)))
                if dp:
                    distributed.all_reduce_gradients(trained, average=not packed)
                if args.max_grad_norm is not None:
                    torch.nn.utils.clip_grad_norm_(self.model.parameters(), args.max_grad_norm)
                optimizer.step()
                self.model.zero_grad()

            def packed_group(group, batch_ix, backprop):
                """The batches of one optimiser step through ONE launch of each kernel.  ``backprop`` False: the
                leftover batches of an epoch (fewer than --batch_accumulation): their losses count, no step is taken
                (reference :273-310 appends every batch's loss and steps only on full groups)."""
                mine = list(range(rank, len(group), world)) if dp else list(range(len(group)))
                vals_t = torch.zeros(len(group), dtype=torch.float64, device=self.device)
                if mine:
                    pc = pack_batches([group[i] for i in mine], self.device, self.model.max_k, constraints_fn=train_cons,
                                      additional_ends_fn=lambda b: self.make_additional_allowed_ends(b['task_name'], b['lengths']))
                    with torch.set_grad_enabled(backprop):
                        loss_b = -self.model.log_likelihood_packed(pc)     # [this rank's batches]
                    if backprop:
                        (loss_b.sum() / len(group)).backward()             # == mean over the step's batches once summed over ranks
                    vals_t[torch.as_tensor(mine, device=self.device)] = loss_b.detach()
                if dp:
                    vals_t = distributed.all_reduce_tensor(vals_t)
                vals = vals_t.cpu().tolist()
                self._check_finite(vals, batch_ix)
                return vals, sum(v * len(b['lengths']) for v, b in zip(vals, group))

            batch_ix = -1
            for batch_ix, batch in enumerate(loader):
                if args.train_limit and batch_ix >= args.train_limit:
                    break
                tasks, lengths = batch['task_name'], batch['lengths']
                num_frames += int(lengths.sum())
                num_videos += len(lengths)
                if packed:
                    pending.append(batch)
                    if len(pending) >= args.batch_accumulation:
                        vals, nll = packed_group(pending, batch_ix, True)
                        losses += vals
                        train_nll += nll
                        pending = []
                        step(batch_ix)
                    continue
                cons = train_cons(batch) if train_cons else None
                features = batch['features'].to(self.device)
                spans = semimarkov_utils.labels_to_spans(batch['gt_single'], max_k=k) if use_labels else None
                addl = self.make_additional_allowed_ends(tasks, lengths)
                ll, log_det = self.model.log_likelihood(features, lengths, valid_classes_per_instance=batch['task_indices'],
                                                        spans=spans, add_eos=True, use_mean_z=use_labels,
                                                        additional_allowed_ends_per_instance=addl, constraints=cons)
                loss = -ll - log_det
                pending.append(loss)
                # data parallel without a packed step: every rank runs the batch; the scalars that steer the run (finiteness
                # check, scheduler, snapshot selection) are rank 0's, so the ranks cannot drift apart on a last-bit difference
                lv = torch.stack([loss.detach().double(), (-ll).detach().double()])
                if dp:
                    lv = distributed.broadcast_tensor(lv, src=0)
                lv = lv.tolist()
                losses.append(lv[0])
                self._check_finite(losses[-1:], batch_ix)
                train_nll += lv[1] * len(lengths)
                if len(pending) >= args.batch_accumulation:
                    (sum(pending) / len(pending)).backward()
                    pending = []
                    step(batch_ix)
            if packed and pending:
                vals, nll = packed_group(pending, batch_ix, False)
                losses += vals
                train_nll += nll
                pending = []
            train_loss = float(np.mean(losses))
            if scheduler is not None:
                scheduler.step(train_loss)
            if callback_fn:
                callback_fn(epoch, {'train_loss': train_loss, 'train_nll_frame_avg': train_nll / max(num_frames, 1),
                                    'train_kl_vid_avg': 0.0, 'train_recon_bound': train_nll / max(num_frames, 1)})

    @staticmethod
    def _check_finite(values, batch_ix):
        """A NaN / inf that reaches the DP kernels (features, or parameters that diverged) comes back as a non-finite
        log-likelihood: stop instead of stepping the optimiser on it."""
        if not all(np.isfinite(v) for v in values):
            raise FloatingPointError("non-finite training loss %s at batch %d (NaN / inf in the features or the "
                                     "parameters reached the log-partition kernels)" % (values, batch_ix))

    # ------------------------------------------------------------------ constraints (reference :135-157)
    def make_additional_allowed_ends(self, tasks, lengths):
        if self.ordered_indices_by_task is None:
            return None
        res = []
        for task, length in zip(tasks, lengths):
            order = self.ordered_indices_by_task[task]
            n = int(length)
            res.append([order[n - 1]] if n < len(order) else [])
        return res

    def expand_constraints(self, datasplit, task, task_indices, constraints):
        """b x T x S step constraints -> b x T x C in the task's class order, zeros on the background columns (reference
        :149-157).  Stays on the device of ``constraints``: one scatter instead of a column loop."""
        task_indices = [int(v) for v in task_indices]
        step_indices = datasplit.get_ordered_indices_no_background()[task]
        assert constraints.size(2) == len(step_indices)
        cache = self.__dict__.setdefault('_step_columns', {})
        key = (task, tuple(task_indices), str(constraints.device))
        cols = cache.get(key)
        if cols is None:
            cols = cache[key] = torch.tensor([task_indices.index(label) for label in step_indices], dtype=torch.long,
                                             device=constraints.device)
        out = torch.zeros((constraints.size(0), constraints.size(1), len(task_indices)), dtype=constraints.dtype,
                          device=constraints.device)
        out[:, :, cols] = constraints
        return out

    def _train_constraints(self, train_data):
        if 'train' not in self.args.sm_constrain_with_narration:
            return None

        def fn(batch):
            tasks = batch['task_name']
            assert all_equal(tasks)
            cons = batch['constraints'].to(self.device, non_blocking=True)     # (S columns: expanded on the device)
            ce = self.expand_constraints(train_data, tasks[0], batch['task_indices'][0], 1 - cons)
            return ce * self.args.sm_constrain_narration_weight
        return fn

    def _test_constraints(self, test_data):
        if 'test' not in self.args.sm_constrain_with_narration:
            return None

        def fn(batch):
            tasks = batch['task_name']
            assert all_equal(tasks)
            cons = batch['constraints'].to(self.device, non_blocking=True)
            ce = self.expand_constraints(test_data, tasks[0], batch['task_indices'][0], 1 - cons)
            return ce * self.args.sm_constrain_narration_weight
        return fn

    # ------------------------------------------------------------------ decode (reference :318-410)
    # A datasplit that is decoded again and again -- the training loop decodes train + dev after EVERY epoch
    # (reference main.py:207-244) -- is collated, packed and uploaded once and kept resident in HBM (288 GB: the features
    # of a whole corpus fit many times over); only the factor tables are rebuilt from the current parameters.
    # ``cache_prepared_bytes`` bounds what may stay resident (0 switches the cache off).
    cache_prepared_bytes = 64 << 30

    def prepare(self, test_data, shard=None):
        """Everything that happens before the timed decode: collate the reference's batches, move them to the
        device once, stack the per-task factor tables.  ``shard=(rank, world)``: this rank's share of the batches
        (multi-GPU decode: videos are independent, every rank decodes its own; batching.make_data_loader)."""
        # everything baked into the cached PackedCorpus (constraints scaled by the narration weight, K clipped per batch,
        # end penalties from the allowed-ends tables) is part of the key
        key = self._prepared_key(test_data, shard)
        cache = self.__dict__.setdefault('_prepared', {})
        hit = cache.get(key)
        if hit is not None and hit[0]() is test_data:
            return self.model.prepare_packed(hit[1])        # (rebuilds the tables; the rest of the corpus is static)
        loader = make_data_loader(self.args, test_data, shuffle=False, batch_by_task=True, batch_size=self.args.batch_size,
                                  shard=shard)
        pc = pack_batches(loader, self.device, self.model.max_k, constraints_fn=self._test_constraints(test_data),
                          additional_ends_fn=lambda b: self.make_additional_allowed_ends(b['task_name'], b['lengths']))
        resident = lambda q: q.x.numel() * 4 + sum(c.numel() * 4 for c in (getattr(q, 'cons_list', None) or []) if c is not None)
        nbytes = resident(pc)
        if nbytes <= self.cache_prepared_bytes:
            import weakref
            held = sum(resident(v[1]) for v in cache.values())
            if held + nbytes > self.cache_prepared_bytes:
                cache.clear()
            try:
                cache[key] = (weakref.ref(test_data), pc)
            except TypeError:                               # (a datasplit type that cannot be weakly referenced)
                pass
        return self.model.prepare_packed(pc)

    def _prepared_key(self, test_data, shard, *extra):
        """Everything baked into a cached PackedCorpus: the datasplit (by identity -- the cache holds a weak reference and
        checks it), the shard, the narration constraints and their weight, K (clipped per batch), the allowed-ends
        tables, the task orderings, the batching and the device."""
        order = self.ordered_indices_by_task
        return (id(test_data), len(test_data), shard, tuple(self.args.sm_constrain_with_narration),
                float(getattr(self.args, 'sm_constrain_narration_weight', 0.0)), self.model.max_k,
                None if self.model.allowed_ends is None else tuple(sorted(self.model.allowed_ends)),
                None if order is None else tuple((t, tuple(v)) for t, v in sorted(order.items())),
                self.args.batch_size, str(self.device)) + tuple(extra)

    def clear_prepared(self):
        """Drop every datasplit kept resident by ``prepare`` (frees the HBM they hold)."""
        self.__dict__.pop('_prepared', None)

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('_prepared', None)                        # device-resident copies of datasets are not model state
        state.pop('_prepared_host', None)
        state.pop('_host_stream_state', None)
        state.pop('_step_columns', None)
        return state

    @staticmethod
    def _per_video(pc, by_video, missing):
        """The values of ``by_video`` for the videos of ``pc``, in the order of ``pc.video_names``; ValueError ``missing`` (a
        text with one place for the name) for the first video without one."""
        absent = [name for name in pc.video_names if name not in by_video]
        if absent:
            raise ValueError(missing % (absent[0],))
        return [by_video[name] for name in pc.video_names]

    def _labels_by_video(self, pc, labels, what='alignments'):
        """Frame labels on the packed frame axis, [total_frames] or [n_samples, total_frames], to the host -> {video: its
        frames' int64 [T] or [n_samples, T]}."""
        lab = labels.cpu().numpy()
        assert lab.size == 0 or int(lab.max()) < self.model.n_classes, "%s should not contain EOS" % what
        return {name: lab[..., off:off + t] for name, off, t in zip(pc.video_names, pc.frame_offset, pc.lengths)}

    def _predict_mbr(self, test_data, fused, shard):
        """``predict(decoder='mbr')``: the minimum-Bayes-risk segmentation under frame loss of every video."""
        if fused:
            pc = self.prepare(test_data, shard=shard)
            if pc.n_videos == 0:
                return {}                                   # this rank's shard is empty
            self.last_predict_path = 'fused MBR: posteriors + smm_mbr_f64 on the packed corpus'
            return self._labels_by_video(pc, self.model.mbr_decode_packed(pc)[0], 'predictions')
        self.last_predict_path = 'per batch, padded: mbr_decode() spans'
        cons_fn = self._test_constraints(test_data)
        loader = make_data_loader(self.args, test_data, shuffle=False, batch_by_task=True, batch_size=self.args.batch_size,
                                  shard=shard)
        predictions = {}
        for batch in loader:
            tasks = batch['task_name']
            assert len(set(tasks)) == 1
            features, lengths = batch['features'].to(self.device), batch['lengths']
            cons = cons_fn(batch) if cons_fn else None
            addl = self.make_additional_allowed_ends(tasks, lengths)
            spans, _ = self.model.mbr_decode(features, lengths, batch['task_indices'], add_eos=True,
                                             additional_allowed_ends_per_instance=addl, constraints=cons)
            pred_labels = semimarkov_utils.spans_to_labels(spans)
            for video, seq in zip(batch['video_name'], self.model.trim(pred_labels, batch['lengths'], check_eos=True)):
                predictions[video] = seq.numpy()
                assert self.model.n_classes not in predictions[video], "predictions should not contain EOS"
        return predictions

    def segment_confidence(self, data, labels_by_video=None, shard=None):
        """``{video: [(start, end, class id, probability, probability of a boundary at start), ...]}``: how sure the model is of
        each segment of a labelling, exactly.  ``labels_by_video[name]``: the video's frame labels (global class ids, one per
        frame), as ``predict`` returns them; None: ``predict``'s own.  The labels become segments the way the training labels
        do (``labels_to_spans``: a run of one label is one segment, cut every span limit - 1 frames, the limit being the
        video's own); a segment covers the frames [start, end).  ``probability`` is the posterior probability that exactly this
        segment -- class, start and end -- is part of the segmentation (0 for a segment the lattice does not have, such as a
        class outside the video's task); the last entry is the posterior probability that a segment of any class starts at
        ``start``.  One emission launch, one log Z launch and one smm_segment_posteriors_f64 launch on the packed corpus
        (``SemiMarkovModule.segment_posteriors_packed``).  Values, not differentiable."""
        self.model.eval()
        pc = self.prepare(data, shard=shard)
        if pc.n_videos == 0:
            return {}
        if labels_by_video is None:
            labels_by_video = self.predict_packed(pc)
        labels = self._per_video(pc, labels_by_video, "segment_confidence: no labels for video %r")
        batch = pc.batch
        spans = np.full((pc.n_videos, batch.t_max + 1), -1, dtype=np.int64)
        for i, (name, lab, t) in enumerate(zip(pc.video_names, labels, batch.lengths.tolist())):
            lab = np.asarray(lab, dtype=np.int64).reshape(-1)
            if lab.shape[0] != t:
                raise ValueError("segment_confidence: video %r has %d frames, %d labels were given" % (name, t, lab.shape[0]))
            if lab.size and int(lab.min()) < 0:
                raise ValueError("segment_confidence: video %r has a negative label" % (name,))
            kp = int(batch.kp[i]) if batch.kp is not None else min(batch.k_rows, batch.t_max)
            spans[i, :t] = semimarkov_utils.labels_to_spans(lab[None], max_k=kp)[0]
            spans[i, t] = self.model.n_classes                 # the EOS position closes the last segment
        out = self.model.segment_posteriors_packed(pc, torch.from_numpy(spans))
        prob = torch.exp(out['seg_logp']).cpu().numpy()
        bnd = out['boundary'].cpu().numpy()
        result = {}
        for i, (name, off, t) in enumerate(zip(pc.video_names, pc.frame_offset, batch.lengths.tolist())):
            starts = np.flatnonzero(spans[i, :t] != -1)
            ends = np.append(starts[1:], t)
            result[name] = [(int(s), int(e), int(spans[i, s]), float(prob[i, s]), float(bnd[int(off) + s]))
                            for s, e in zip(starts, ends)]
        return result

    def expected_accuracy(self, data, labels_by_video=None, shard=None):
        """``{video: expected number of frames on which a segmentation drawn from the posterior agrees with the labels}``,
        exactly.  ``labels_by_video[name]``: the video's frame labels (global class ids, one per frame), as ``predict`` returns
        them; None: the ground truth of ``data`` (``gt_single``).  A label outside the video's task is never correct.  Against
        ``predict(decoder='mbr')``'s labels it is the calibrated estimate of that decode's frame accuracy.  One emission launch,
        one log Z launch and one smm_expected_reward_f64 launch on the packed corpus
        (``SemiMarkovModule.expected_accuracy_packed``).  Values, not differentiable."""
        self.model.eval()
        pc = self.prepare(data, shard=shard)
        if pc.n_videos == 0:
            return {}
        packed = self._packed_labels(pc, data, labels_by_video, 'expected_accuracy')
        with torch.no_grad():
            v = self.model.expected_accuracy_packed(pc, packed).cpu().numpy()
        return {name: float(x) for name, x in zip(pc.video_names, v)}

    def _packed_labels(self, pc, data, labels_by_video, what):
        """``labels_by_video`` (None: the ground truth of ``data``, ``gt_single``) on the packed frame axis of ``pc``: int64
        total_frames, -1 on frames no video covers."""
        if labels_by_video is None:
            loader = make_data_loader(self.args, data, batch_by_task=False, shuffle=False, batch_size=1)
            labels_by_video = {batch['video_name'][0]: batch['gt_single'].squeeze(0).cpu().numpy() for batch in loader}
        labels = self._per_video(pc, labels_by_video, what + ": no labels for video %r")
        batch = pc.batch
        packed = np.full(batch.total_frames, -1, dtype=np.int64)
        for name, lab, off, t in zip(pc.video_names, labels, pc.frame_offset, batch.lengths.tolist()):
            lab = np.asarray(lab, dtype=np.int64).reshape(-1)
            if lab.shape[0] != t:
                raise ValueError("%s: video %r has %d frames, %d labels were given" % (what, name, t, lab.shape[0]))
            packed[int(off):int(off) + t] = lab
        return torch.from_numpy(packed)

    def alignment_expected_accuracy(self, data, transcripts_by_video, labels_by_video=None, shard=None, *, optional_by_video=None,
                                    optional_classes=None):
        """``{video: expected number of frames on which an alignment drawn from the posterior given the video's transcript agrees
        with the labels}``, exactly (``align``'s conventions for ``transcripts_by_video``, ``optional_by_video`` and
        ``optional_classes``; ``expected_accuracy``'s for ``labels_by_video``, None: the ground truth of ``data``).  The frame
        accuracy weak supervision can reach without committing to the best alignment; NaN where the transcript cannot be laid
        over the video.  One emission launch, the forward launch and one smm_align_graph_expected_reward_f64 launch on the
        packed corpus (``SemiMarkovModule.alignment_expected_accuracy_packed``).  Values, not differentiable."""
        from . import ops
        self._one_kind_of_flags(optional_by_video, optional_classes, 'alignment_expected_accuracy')
        self.model.eval()
        pc = self.prepare(data, shard=shard)
        if pc.n_videos == 0:
            return {}
        transcripts = self._per_video(pc, transcripts_by_video, "alignment_expected_accuracy: no transcript for video %r")
        optional = self._optional_flags(pc, transcripts, optional_by_video, optional_classes, 'alignment_expected_accuracy')
        if optional is None:
            graphs = [ops.TranscriptGraph.chain(t) for t in transcripts]
        else:
            graphs = [ops.TranscriptGraph.from_optional(t, f) for t, f in zip(transcripts, optional)]
        packed = self._packed_labels(pc, data, labels_by_video, 'alignment_expected_accuracy')
        with torch.no_grad():
            v = self.model.alignment_expected_accuracy_packed(pc, graphs, packed).cpu().numpy()
        return {name: float(x) for name, x in zip(pc.video_names, v)}

    def candidate_expected_accuracy(self, data, candidates_by_video, labels_by_video=None, shard=None):
        """``alignment_expected_accuracy`` given "the video follows one of these transcripts" (``candidates_by_video`` as in
        ``align_candidates``): the expectation under the joint posterior over candidate and boundaries, which is the sum over
        the candidates of ``candidate_posteriors`` times the candidate's own expected accuracy.  One prefix trie per video:
        ValueError as ``candidate_entropy``."""
        from . import ops
        self._one_trie_each(candidates_by_video, 'candidate_expected_accuracy')
        self.model.eval()
        pc = self.prepare(data, shard=shard)
        if pc.n_videos == 0:
            return {}
        graphs = [ops.TranscriptGraph.from_candidates(cands)
                  for cands in self._per_video(pc, candidates_by_video, "candidate_expected_accuracy: no candidates for video %r")]
        packed = self._packed_labels(pc, data, labels_by_video, 'candidate_expected_accuracy')
        with torch.no_grad():
            v = self.model.alignment_expected_accuracy_packed(pc, graphs, packed).cpu().numpy()
        return {name: float(x) for name, x in zip(pc.video_names, v)}

    def expected_segment_counts(self, data, shard=None):
        """``{video: expected number of segments under the posterior}``, exactly
        (``SemiMarkovModule.expected_segment_count_packed``).  Values, not differentiable."""
        self.model.eval()
        pc = self.prepare(data, shard=shard)
        if pc.n_videos == 0:
            return {}
        with torch.no_grad():
            v = self.model.expected_segment_count_packed(pc).cpu().numpy()
        return {name: float(x) for name, x in zip(pc.video_names, v)}

    def align(self, data, transcripts_by_video, shard=None, *, optional_by_video=None, optional_classes=None):
        """Forced alignment of every video of ``data`` to its transcript: ``transcripts_by_video[name]`` is the video's class
        sequence in global class ids, one entry per segment.  Returns what ``predict`` returns, ``{video: int64[T]}``: the frame
        labels of the best segmentation with that class sequence (-1 on a video whose transcript cannot be laid over its
        frames).  One emission launch and one alignment launch on the packed corpus (``SemiMarkovModule.align_packed``).

        Entries may be optional: the result is then the best segmentation whose class sequence is the transcript with any
        subset of the optional entries left out.  ``optional_by_video[name]``: one boolean per entry of the video's
        transcript; or ``optional_classes``: an iterable of global class ids, every entry of such a class being optional
        (a CrossTask task ``bg, step_1, bg, ...``: pass the background ids).  ValueError when both are given."""
        self._one_kind_of_flags(optional_by_video, optional_classes, 'align')
        self.model.eval()
        pc = self.prepare(data, shard=shard)
        if pc.n_videos == 0:
            return {}
        transcripts = self._per_video(pc, transcripts_by_video, "align: no transcript for video %r")
        optional = self._optional_flags(pc, transcripts, optional_by_video, optional_classes, 'align')
        return self._labels_by_video(pc, self.model.align_packed(pc, transcripts, optional=optional)[0])

    def align_candidates(self, data, candidates_by_video, shard=None):
        """"The video follows one of these transcripts": ``candidates_by_video[name]`` is a list of class sequences in global
        class ids.  Returns ``({video: int64[T] frame labels}, {video: index of the chosen candidate})``: the best segmentation
        over every candidate, and which one it follows; labels -1 and index -1 where no candidate can be laid over the video.
        The candidates of a video go to the GPU as their prefix trie (``ops.TranscriptGraph.from_candidates``,
        ``SemiMarkovModule.align_graph_packed``): one launch scores all of them, shared prefixes once.  A list whose trie would
        exceed ``ops.MAX_TRANSCRIPT`` nodes is split into consecutive tries (``_candidate_chunks``: its distinct candidates,
        packed greedily in candidate order), each aligned by its own launch on the same prepared corpus; a strictly better
        score replaces the earlier one on the device, so a tie keeps the earlier trie, and identical candidates answer to the
        lowest index.  ValueError for a video without candidates, an empty candidate or one longer than
        ``ops.MAX_TRANSCRIPT``.  Under an exact tie between different candidates the chosen index is deterministic but
        otherwise unspecified."""
        pc, rounds = self._candidate_rounds(data, candidates_by_video, shard, 'align_candidates')
        if pc.n_videos == 0:
            return {}, {}
        labels = scores = None
        for row in rounds:
            # (a video all of whose tries went out earlier repeats its last one: the same score never replaces)
            lab, sc, used = self.model.align_graph_packed(pc, [trie for trie, _, _ in row])
            ends = [np.flatnonzero(u.cpu().numpy()) for u in used]          # the path's nodes; the last one is its end
            idx = np.array([owner[e[-1]] if e.size else -1 for (_, owner, _), e in zip(row, ends)], np.int64)
            if labels is None:
                labels, scores, chosen = lab, sc, idx
                # the packed frame axis: which video a covered frame belongs to
                where = torch.cat([torch.arange(off, off + t, device=lab.device) for off, t in zip(pc.frame_offset, pc.lengths)])
                video = torch.repeat_interleave(torch.arange(pc.n_videos, device=lab.device),
                                                torch.as_tensor(np.asarray(pc.lengths, np.int64), device=lab.device))
                continue
            better = sc > scores                            # (strictly: a tie keeps the earlier trie)
            labels[where] = torch.where(better[video], lab[where], labels[where])
            scores = torch.where(better, sc, scores)
            chosen = np.where(better.cpu().numpy(), idx, chosen)
        return self._labels_by_video(pc, labels), {name: int(c) for name, c in zip(pc.video_names, chosen)}

    @staticmethod
    def _candidate_chunks(cands, name, what):
        """The DISTINCT candidates of one video, each under the index of its first appearance, split into consecutive tries of
        at most ``ops.MAX_TRANSCRIPT`` nodes, packed greedily in candidate order.  De-duplicating first keeps a class sequence
        from being summed once per chunk it would appear in.
        -> [[(index, class sequence)]], one list per trie."""
        from . import ops
        if not cands:
            raise ValueError("%s: no candidates for video %r" % (what, name))
        chunks, cur, seen, known = [], [], set(), set()
        for ci, cand in enumerate(cands):
            seq = tuple(int(c) for c in np.asarray(cand.cpu() if torch.is_tensor(cand) else cand, dtype=np.int64).reshape(-1))
            if len(seq) == 0 or len(seq) > ops.MAX_TRANSCRIPT:
                raise ValueError("%s: candidate %d of video %r has %d entries (1 to %d)" % (what, ci, name, len(seq), ops.MAX_TRANSCRIPT))
            if seq in known:
                continue
            known.add(seq)
            prefixes = {seq[:n] for n in range(1, len(seq) + 1)}
            if cur and len(seen | prefixes) > ops.MAX_TRANSCRIPT:
                chunks.append(cur)
                cur, seen = [], set()
            cur.append((ci, seq))
            seen |= prefixes
        chunks.append(cur)
        return chunks

    def _candidate_rounds(self, data, candidates_by_video, shard, what):
        """-> (pc, rounds): the prepared corpus and, per launch, one (trie, owner, fresh) triple per video -- owner[node]: the
        index of the candidate that ends in the node, else -1; fresh: False for a video all of whose tries went out in earlier
        launches (it then repeats its last trie: a sum leaves the launch's values for it out, a maximum is not moved by them)."""
        from . import ops
        self.model.eval()
        chunks = {name: self._candidate_chunks(cands, name, what) for name, cands in candidates_by_video.items()}
        pc = self.prepare(data, shard=shard)
        if pc.n_videos == 0:
            return pc, []
        chunks = self._per_video(pc, chunks, what + ": no candidates for video %r")
        rounds = []
        for r in range(max(len(mine) for mine in chunks)):
            row = []
            for mine in chunks:
                part = mine[min(r, len(mine) - 1)]
                trie = ops.TranscriptGraph.from_candidates([seq for _, seq in part])
                owner = np.where(trie.end_candidate >= 0, np.array([ci for ci, _ in part], np.int64)[trie.end_candidate], -1)
                row.append((trie, owner, r < len(mine)))
            rounds.append(row)
        return pc, rounds

    def candidate_log_likelihood(self, data, candidates_by_video, conditional=False, shard=None):
        """The likelihood of "the video follows one of these transcripts": ``candidates_by_video[name]`` is a list of class
        sequences in global class ids.  Returns ``{video: float}``: the log of the sum, over the DISTINCT candidates, of the
        sum over every segmentation with that class sequence (``conditional``: minus log Z, the log-probability that the
        video's class sequence is one of the candidates); -inf where no candidate can be laid over the video.  The candidates
        go to the GPU as their prefix trie (``SemiMarkovModule.transcript_graph_scores_packed``): shared prefixes are summed
        once.  A set whose trie would exceed ``ops.MAX_TRANSCRIPT`` nodes is split as ``align_candidates`` splits it, after
        de-duplication, and the tries' values are combined by logsumexp."""
        pc, rounds = self._candidate_rounds(data, candidates_by_video, shard, 'candidate_log_likelihood')
        if pc.n_videos == 0:
            return {}
        total = torch.full((pc.n_videos,), float('-inf'), dtype=torch.float64)
        for row in rounds:
            z = self.model.transcript_graph_scores_packed(pc, [t for t, _, _ in row], conditional=conditional)
            live = torch.tensor([fresh for _, _, fresh in row])
            total = torch.logaddexp(total, torch.where(live, z, torch.full_like(z, float('-inf'))))
        return {name: float(v) for name, v in zip(pc.video_names, total.tolist())}

    def candidate_posteriors(self, data, candidates_by_video, shard=None):
        """``{video: fp64 [n_candidates]}``: the posterior probability of each candidate transcript given the frames and "the
        video follows one of them" -- log Z_a of the candidate minus the candidates' logsumexp, exponentiated; it adds up to 1.
        Identical candidates share one class sequence and so one mass: it goes to the one with the lowest index, the others
        get 0.  All zeros where no candidate can be laid over the video.  One forward and one backward launch per trie
        (``SemiMarkovModule.transcript_node_posteriors_packed``: the end posteriors of the trie's nodes); a set split into
        several tries weighs each trie by its share of the total."""
        pc, rounds = self._candidate_rounds(data, candidates_by_video, shard, 'candidate_posteriors')
        if pc.n_videos == 0:
            return {}
        out = [np.zeros(len(candidates_by_video[name])) for name in pc.video_names]
        zs = []
        for row in rounds:
            graphs = [t for t, _, _ in row]
            z = self.model.transcript_graph_scores_packed(pc, graphs).numpy()
            _, p_end = self.model.transcript_node_posteriors_packed(pc, graphs)
            zs.append(np.where([fresh for _, _, fresh in row], z, -np.inf))
            for i, (_, owner, fresh) in enumerate(row):
                if fresh and np.isfinite(z[i]):
                    ends = owner >= 0
                    out[i][owner[ends]] = p_end[i][ends]            # (within the trie; weighed below)
        zs = np.array(zs)                                           # [launches, videos]
        top = zs.max(axis=0)
        with np.errstate(invalid='ignore'):
            share = np.where(np.isfinite(top), np.exp(zs - np.where(np.isfinite(top), top, 0.0)), 0.0)
        share = share / np.maximum(share.sum(axis=0), 1e-300)
        for r, row in enumerate(rounds):
            for i, (_, owner, fresh) in enumerate(row):
                if fresh:
                    out[i][owner[owner >= 0]] *= share[r, i]
        return dict(zip(pc.video_names, out))

    def sample_alignments(self, data, transcripts_by_video, n_samples, seed=0, shard=None, *, optional_by_video=None,
                          optional_classes=None):
        """Alignments of every video of ``data`` drawn from the posterior given its transcript (``align``'s conventions for
        ``transcripts_by_video``, ``optional_by_video`` and ``optional_classes``): where the boundaries lie and, with optional
        entries, which of them are kept.  Returns ``{video: int64 [n_samples, T]}`` frame labels -- pseudo-labels for
        ``fit_supervised`` (stochastic EM from transcripts) --, rows of -1 where the transcript cannot be laid over the video.
        Sample j depends on (seed, video, j) only.  One emission launch, the forward launch and the sampler on the packed
        corpus (``SemiMarkovModule.sample_alignments_packed``)."""
        from . import ops
        self._one_kind_of_flags(optional_by_video, optional_classes, 'sample_alignments')
        if int(n_samples) < 1:
            raise ValueError("sample_alignments: n_samples must be positive, got %d" % int(n_samples))
        self.model.eval()
        pc = self.prepare(data, shard=shard)
        if pc.n_videos == 0:
            return {}
        transcripts = self._per_video(pc, transcripts_by_video, "sample_alignments: no transcript for video %r")
        optional = self._optional_flags(pc, transcripts, optional_by_video, optional_classes, 'sample_alignments')
        if optional is None:
            graphs = [ops.TranscriptGraph.chain(t) for t in transcripts]
        else:
            graphs = [ops.TranscriptGraph.from_optional(t, f) for t, f in zip(transcripts, optional)]
        return self._labels_by_video(pc, self.model.sample_alignments_packed(pc, graphs, n_samples, seed=seed)[0])

    def sample_candidates(self, data, candidates_by_video, n_samples, seed=0, shard=None):
        """Joint draws of which candidate transcript a video follows and where its boundaries lie, from the posterior given
        the frames and "the video follows one of them" (``candidates_by_video`` as in ``align_candidates``).  Returns
        ``({video: int64 [n_samples, T] frame labels}, {video: int64 [n_samples] candidate index})``; identical candidates
        map to the lowest index, as in ``candidate_posteriors``; labels and index -1 where no candidate can be laid over the
        video.  The candidates go to the GPU as one prefix trie per video: ValueError for a set whose trie needs more than
        ``ops.MAX_TRANSCRIPT`` nodes (a draw across several tries is not offered)."""
        from . import ops
        if int(n_samples) < 1:
            raise ValueError("sample_candidates: n_samples must be positive, got %d" % int(n_samples))
        self._one_trie_each(candidates_by_video, 'sample_candidates')
        self.model.eval()
        pc = self.prepare(data, shard=shard)
        if pc.n_videos == 0:
            return {}, {}
        graphs = [ops.TranscriptGraph.from_candidates(cands)
                  for cands in self._per_video(pc, candidates_by_video, "sample_candidates: no candidates for video %r")]
        labels, _, used = self.model.sample_alignments_packed(pc, graphs, n_samples, seed=seed)
        chosen = {}
        for name, g, u in zip(pc.video_names, graphs, used):
            u = u.cpu().numpy() != 0                               # [n_samples, M]; the end node is the last used one
            last = u.shape[1] - 1 - np.argmax(u[:, ::-1], axis=1)
            chosen[name] = np.where(u.any(axis=1), g.end_candidate[last], -1).astype(np.int64)
        return self._labels_by_video(pc, labels), chosen

    def alignment_entropy(self, data, transcripts_by_video, shard=None, *, optional_by_video=None, optional_classes=None):
        """``{video: float}``: the exact entropy, in nats, of the posterior ``sample_alignments`` draws from -- how sure the
        model is of where the boundaries of the video's transcript lie and, with optional entries, of which are kept
        (``align``'s conventions for ``transcripts_by_video``, ``optional_by_video`` and ``optional_classes``).  0 when one
        alignment has all the mass; NaN where the transcript cannot be laid over the video.  Ranks weakly labelled videos for
        annotation and selects pseudo-labels for ``fit_supervised``.  One emission launch, the forward launch and the entropy
        launch on the packed corpus (``SemiMarkovModule.alignment_entropy_packed``)."""
        from . import ops
        self._one_kind_of_flags(optional_by_video, optional_classes, 'alignment_entropy')
        self.model.eval()
        pc = self.prepare(data, shard=shard)
        if pc.n_videos == 0:
            return {}
        transcripts = self._per_video(pc, transcripts_by_video, "alignment_entropy: no transcript for video %r")
        optional = self._optional_flags(pc, transcripts, optional_by_video, optional_classes, 'alignment_entropy')
        if optional is None:
            graphs = [ops.TranscriptGraph.chain(t) for t in transcripts]
        else:
            graphs = [ops.TranscriptGraph.from_optional(t, f) for t, f in zip(transcripts, optional)]
        return dict(zip(pc.video_names, self.model.alignment_entropy_packed(pc, graphs).tolist()))

    def _alignment_confidence(self, pc, graphs):
        """The best alignment of every video of ``pc`` to its graph with the exact posterior of each of its segments:
        ``{video: [(node index, class id, start, end, probability, end_mean, end_sd), ...]}``."""
        out = self.model.alignment_segment_posteriors_packed(pc, graphs)
        spans = out['spans'].cpu().numpy()
        prob = torch.exp(out['seg_logp']).cpu().numpy()
        result = {}
        for i, (name, t) in enumerate(zip(pc.video_names, pc.batch.lengths.tolist())):
            nodes = np.flatnonzero(out['used'][i].cpu().numpy())
            starts = np.flatnonzero(spans[i, :t] != -1)
            mean, sd = out['end_mean'][i].cpu().numpy(), out['end_sd'][i].cpu().numpy()
            result[name] = [(int(m), int(spans[i, s]), int(s), int(e), float(prob[i, s]), float(mean[m]), float(sd[m]))
                            for m, s, e in zip(nodes, starts, np.append(starts[1:], t))]
        return result

    def alignment_confidence(self, data, transcripts_by_video, shard=None, *, optional_by_video=None, optional_classes=None):
        """``{video: [(entry index, class id, start, end, probability, end_mean, end_sd), ...]}``: the best alignment of every
        video to its transcript (``align``'s conventions for ``transcripts_by_video``, ``optional_by_video`` and
        ``optional_classes``), one row per entry that got a segment, on the frames [start, end).  ``probability`` is the exact
        posterior probability, under the distribution ``sample_alignments`` draws from, that this entry covers exactly these
        frames; ``end_mean`` and ``end_sd`` are the mean and the standard deviation, in frames, of where the entry's segment
        ends, given that the entry is kept.  An empty list where the transcript cannot be laid over the video.  One emission
        launch, one alignment launch, the forward launch and one smm_align_graph_segment_posteriors_f64 launch on the packed
        corpus (``SemiMarkovModule.alignment_segment_posteriors_packed``).  Values, not differentiable."""
        from . import ops
        self._one_kind_of_flags(optional_by_video, optional_classes, 'alignment_confidence')
        self.model.eval()
        pc = self.prepare(data, shard=shard)
        if pc.n_videos == 0:
            return {}
        transcripts = self._per_video(pc, transcripts_by_video, "alignment_confidence: no transcript for video %r")
        optional = self._optional_flags(pc, transcripts, optional_by_video, optional_classes, 'alignment_confidence')
        if optional is None:
            graphs = [ops.TranscriptGraph.chain(t) for t in transcripts]
        else:
            graphs = [ops.TranscriptGraph.from_optional(t, f) for t, f in zip(transcripts, optional)]
        return self._alignment_confidence(pc, graphs)

    def candidate_confidence(self, data, candidates_by_video, shard=None):
        """``alignment_confidence`` given "the video follows one of these transcripts" (``candidates_by_video`` as in
        ``align_candidates``): the rows of the best alignment over every candidate, the first entry of a row being the node of
        the candidates' prefix trie (``ops.TranscriptGraph.from_candidates``); the probabilities are under the joint posterior
        over candidate and boundaries.  ValueError for an empty set or one whose trie needs more than ``ops.MAX_TRANSCRIPT``
        nodes, as in ``candidate_entropy``."""
        from . import ops
        self._one_trie_each(candidates_by_video, 'candidate_confidence')
        self.model.eval()
        pc = self.prepare(data, shard=shard)
        if pc.n_videos == 0:
            return {}
        graphs = [ops.TranscriptGraph.from_candidates(cands)
                  for cands in self._per_video(pc, candidates_by_video, "candidate_confidence: no candidates for video %r")]
        return self._alignment_confidence(pc, graphs)

    def candidate_entropy(self, data, candidates_by_video, shard=None):
        """``{video: dict(total=, candidates=, boundaries=)}`` in nats, given the frames and "the video follows one of these
        transcripts" (``candidates_by_video`` as in ``align_candidates``): the entropy of the joint posterior over candidate and
        boundaries, of ``candidate_posteriors`` -- is the candidate set decided? --, and their difference, the expected entropy
        of the boundaries given the candidate.  NaN where no candidate can be laid over the video.  The candidates go to the
        GPU as one prefix trie per video: ValueError for an empty set or one whose trie needs more than ``ops.MAX_TRANSCRIPT``
        nodes, as in ``sample_candidates``."""
        from . import ops
        self._one_trie_each(candidates_by_video, 'candidate_entropy')
        self.model.eval()
        pc = self.prepare(data, shard=shard)
        if pc.n_videos == 0:
            return {}
        graphs = [ops.TranscriptGraph.from_candidates(cands)
                  for cands in self._per_video(pc, candidates_by_video, "candidate_entropy: no candidates for video %r")]
        h, parts = self.model.alignment_entropy_packed(pc, graphs, want_parts=True)
        return {name: dict(total=t, candidates=e, boundaries=t - e)
                for name, t, e in zip(pc.video_names, h.tolist(), parts[:, 0].tolist())}

    @staticmethod
    def _other_module(other, what):
        if not isinstance(other, SemiMarkovModel):
            raise TypeError("%s: other must be a SemiMarkovModel" % what)
        other.model.eval()
        return other.model

    def alignment_kl(self, other, data, transcripts_by_video, shard=None, *, optional_by_video=None, optional_classes=None):
        """``{video: float}``: the exact KL(p || q), in nats, between this model's posterior over the alignments of each video
        to its transcript and ``other``'s (a SemiMarkovModel on the same lattice; ``alignment_entropy``'s conventions for the
        transcripts and the optional entries): teacher against student, one EM epoch against the next -- it goes to 0 as
        training converges and is exactly 0 against the model itself.  NaN where the transcript cannot be laid over the video,
        +inf where ``other`` excludes an alignment this model does not.  Two emission launches, two forward launches and the KL
        launch on the packed corpus (``SemiMarkovModule.alignment_kl_packed``)."""
        from . import ops
        self._one_kind_of_flags(optional_by_video, optional_classes, 'alignment_kl')
        q = self._other_module(other, 'alignment_kl')
        self.model.eval()
        pc = self.prepare(data, shard=shard)
        if pc.n_videos == 0:
            return {}
        transcripts = self._per_video(pc, transcripts_by_video, "alignment_kl: no transcript for video %r")
        optional = self._optional_flags(pc, transcripts, optional_by_video, optional_classes, 'alignment_kl')
        if optional is None:
            graphs = [ops.TranscriptGraph.chain(t) for t in transcripts]
        else:
            graphs = [ops.TranscriptGraph.from_optional(t, f) for t, f in zip(transcripts, optional)]
        return dict(zip(pc.video_names, self.model.alignment_kl_packed(q, pc, graphs).tolist()))

    def candidate_kl(self, other, data, candidates_by_video, shard=None):
        """``{video: dict(total=, candidates=, boundaries=)}`` in nats, given the frames and "the video follows one of these
        transcripts" (``candidates_by_video`` as in ``candidate_entropy``): the KL between this model's and ``other``'s joint
        posteriors over candidate and boundaries, the KL between their ``candidate_posteriors`` -- do the two models pick the
        same transcript? --, and their difference, the expected KL of the boundaries given the candidate.  NaN where no
        candidate can be laid over the video.  One prefix trie per video: ValueError as ``candidate_entropy``."""
        from . import ops
        self._one_trie_each(candidates_by_video, 'candidate_kl')
        q = self._other_module(other, 'candidate_kl')
        self.model.eval()
        pc = self.prepare(data, shard=shard)
        if pc.n_videos == 0:
            return {}
        graphs = [ops.TranscriptGraph.from_candidates(cands)
                  for cands in self._per_video(pc, candidates_by_video, "candidate_kl: no candidates for video %r")]
        kl, parts = self.model.alignment_kl_packed(q, pc, graphs, want_parts=True)
        return {name: dict(total=t, candidates=e, boundaries=t - e)
                for name, t, e in zip(pc.video_names, kl.tolist(), parts[:, 0].tolist())}

    @staticmethod
    def _one_trie_each(candidates_by_video, what):
        """ValueError for a video without candidates or whose candidates' trie needs more than ``ops.MAX_TRANSCRIPT`` nodes."""
        from . import ops
        for name, cands in candidates_by_video.items():
            if not cands:
                raise ValueError("%s: no candidates for video %r" % (what, name))
            nodes = ops.TranscriptGraph.trie_nodes(cands)
            if nodes > ops.MAX_TRANSCRIPT:
                raise ValueError("%s: the trie of the candidates of video %r has %d nodes (at most %d)"
                                 % (what, name, nodes, ops.MAX_TRANSCRIPT))

    @staticmethod
    def _one_kind_of_flags(optional_by_video, optional_classes, what):
        if optional_by_video is not None and optional_classes is not None:
            raise ValueError("%s: give optional_by_video or optional_classes, not both" % what)

    @staticmethod
    def _refuse_ambiguous(transcripts_by_video, optional_by_video, optional_classes, ambiguous, what):
        """ambiguous='raise', on the host before the corpus is prepared: ValueError naming the first video two subsets of whose
        optional entries give the same class sequence."""
        from . import ops
        if ambiguous not in ('raise', 'allow'):
            raise ValueError("%s: ambiguous must be 'raise' or 'allow'" % what)
        if ambiguous == 'allow' or (optional_by_video is None and optional_classes is None):
            return
        classes = None if optional_classes is None else np.array(sorted(set(int(c) for c in optional_classes)), np.int64)
        for name, t in transcripts_by_video.items():
            ids = np.asarray(t.cpu() if torch.is_tensor(t) else t, dtype=np.int64).reshape(-1)
            if classes is not None:
                flags = np.isin(ids, classes)
            elif name in optional_by_video:
                f = optional_by_video[name]
                flags = np.asarray(f.cpu() if torch.is_tensor(f) else f).reshape(-1) != 0
            else:
                continue
            if flags.size == ids.size and ops.transcript_is_ambiguous(ids, flags):
                raise ValueError("%s: two subsets of the optional entries of video %r give the same class sequence; pass "
                                 "ambiguous='allow' for the sum over alignments" % (what, name))

    @staticmethod
    def _optional_flags(pc, transcripts, optional_by_video, optional_classes, what):
        """The two ways to flag optional entries -> one boolean sequence per video of ``pc`` (None: no flags)."""
        if optional_classes is not None:
            classes = np.array(sorted(set(int(c) for c in optional_classes)), np.int64)
            return [np.isin(np.asarray(t.cpu() if torch.is_tensor(t) else t, dtype=np.int64).reshape(-1), classes)
                    for t in transcripts]
        if optional_by_video is not None:
            return SemiMarkovModel._per_video(pc, optional_by_video, what + ": no optional flags for video %r")
        return None

    def transcript_log_likelihood(self, data, transcripts_by_video, conditional=False, shard=None, *, optional_by_video=None,
                                  optional_classes=None, ambiguous='raise'):
        """The likelihood of every video's transcript: ``transcripts_by_video[name]`` is the video's class sequence in global
        class ids, one entry per segment.  Returns ``{video: float}``: log Z_a, the log of the sum over every segmentation with
        that class sequence (the joint log-likelihood of frames and transcript); ``conditional``: log Z_a - log Z, the
        log-probability of the transcript given the frames.  -inf for a transcript that cannot be laid over its video.  One
        emission launch and the DP launches on the packed corpus (``SemiMarkovModule.transcript_scores_packed``).

        ``optional_by_video`` / ``optional_classes`` (as in ``align``): entries that may be missing; the value is then log Z_o,
        the sum over every alignment with any subset of them left out.  ``ambiguous``: 'raise' -- ValueError naming the first
        video two subsets of whose optional entries give the same class sequence -- or 'allow'."""
        self._one_kind_of_flags(optional_by_video, optional_classes, 'transcript_log_likelihood')
        self._refuse_ambiguous(transcripts_by_video, optional_by_video, optional_classes, ambiguous, 'transcript_log_likelihood')
        self.model.eval()
        pc = self.prepare(data, shard=shard)
        if pc.n_videos == 0:
            return {}
        transcripts = self._per_video(pc, transcripts_by_video, "transcript_log_likelihood: no transcript for video %r")
        optional = self._optional_flags(pc, transcripts, optional_by_video, optional_classes, 'transcript_log_likelihood')
        z = self.model.transcript_scores_packed(pc, transcripts, conditional=conditional, optional=optional, ambiguous=ambiguous)
        return {name: float(v) for name, v in zip(pc.video_names, z.tolist())}

    def transcript_entry_posteriors(self, data, transcripts_by_video, shard=None, *, optional_by_video=None, optional_classes=None,
                                    ambiguous='raise'):
        """``{video: fp64 array}``: per entry of the video's transcript the posterior probability that it has a segment, given
        the frames and the transcript with its optional entries (flagged as in ``align``; 1 for a mandatory entry, zeros for a
        video without an alignment).  ``SemiMarkovModule.transcript_entry_posteriors_packed`` on the packed corpus."""
        self._one_kind_of_flags(optional_by_video, optional_classes, 'transcript_entry_posteriors')
        if optional_by_video is None and optional_classes is None:
            raise ValueError("transcript_entry_posteriors: give optional_by_video or optional_classes")
        self._refuse_ambiguous(transcripts_by_video, optional_by_video, optional_classes, ambiguous, 'transcript_entry_posteriors')
        self.model.eval()
        pc = self.prepare(data, shard=shard)
        if pc.n_videos == 0:
            return {}
        transcripts = self._per_video(pc, transcripts_by_video, "transcript_entry_posteriors: no transcript for video %r")
        optional = self._optional_flags(pc, transcripts, optional_by_video, optional_classes, 'transcript_entry_posteriors')
        post = self.model.transcript_entry_posteriors_packed(pc, transcripts, optional, ambiguous=ambiguous)
        return dict(zip(pc.video_names, post))

    def predict_packed(self, pc):
        import torch
        from . import ops
        if pc.n_videos == 0:
            return {}                                       # this rank's shard is empty
        # the DP kernel writes the labels into pinned host memory while it decodes: synchronise, then they are here -- in a
        # buffer that is OURS until the caller drops the result (ops.lease_host_labels): no copy out of a staging buffer ...
        dev = pc.device or pc.x.device
        lease = ops.lease_host_labels(pc.batch, dev) if dev.type == 'cuda' else None   # (no GPU: decode_packed says so, loudly)
        self.last_predict_path = 'fused: ' + ('leased pinned label buffer' if lease is not None else 'shared staging buffer + copy')
        if lease is not None:
            out = self.model.decode_packed(pc, want_spans=False, want_labels=True, labels_out=lease)
            torch.cuda.current_stream().synchronize()
            lab_t = lease
        else:
            # ... unless LABEL_LEASES earlier results are still alive: then into the shared staging buffer, which the next
            # decode reuses, and the caller gets a copy.  Its pages are fresh from the kernel (20 MB of labels per cfg3
            # decode = 4800 page faults), so they are touched HERE, while the GPU decodes, and the copy behind the
            # synchronisation runs at memcpy speed (torch's fill, copy and reduction run on all host cores)
            out = self.model.decode_packed(pc, want_spans=False, want_labels=True, labels_on_host=True)
            lab_t = torch.empty_like(out['labels'], pin_memory=False).zero_()
            torch.cuda.current_stream().synchronize()
            lab_t.copy_(out['labels'])
        ops.check_decoded(pc.batch, out)
        # one pass over the whole frame axis instead of one scan per video (frames no video covers hold -1)
        assert lab_t.numel() == 0 or int(lab_t.max()) < self.model.n_classes, "predictions should not contain EOS"
        labels = lab_t.numpy()
        return {name: labels[off:off + t] for name, off, t in zip(pc.video_names, pc.frame_offset, pc.lengths)}

    # ------------------------------------------------------------------ host-resident features
    # The reference loads every video's features from disk into host memory (crosstask.py:95-112) and moves each batch
    # of five to the device synchronously (semimarkov.py:349-354).  Here a datasplit whose features stay on the host is
    # packed into a few SLABS of pinned memory once; a decode pass then streams them over PCIe on a copy stream into two
    # device buffers while the previous slab is being decoded (emission + DP read the features once), and the labels
    # leave through the DP kernel's stores into pinned memory: the pass costs about the upload, 4 D bytes per frame.
    def prepare_host(self, test_data, n_slabs=6, shard=None):
        """Collate the reference's batches and pack them into ``n_slabs`` PackedCorpora whose features live in pinned
        host memory (whole single-task batches per slab, balanced by frames).  Done once per datasplit."""
        loader = make_data_loader(self.args, test_data, shuffle=False, batch_by_task=True, batch_size=self.args.batch_size,
                                  shard=shard)
        batches = list(loader)
        # longest videos first: a slab's decode lasts as long as its longest video (the DP is one serial chain per video),
        # and the pass ends with the decode of the LAST slab, which no upload overlaps -- so the last slab gets the
        # batches whose longest video is shortest (round 3 kept the loader's order: a 14 000-frame video in the last
        # slab left 3 ms of a 40 ms pass uncovered)
        batches.sort(key=lambda b: -int(b['lengths'].max()))
        frames = [int(b['lengths'].sum()) for b in batches]
        # equal shares, except that the last two slabs split one share 3 : 1: keep the uncovered decode short
        shares = [1.0] * n_slabs if n_slabs < 3 else [1.0] * (n_slabs - 2) + [0.75, 0.25]
        bounds = np.cumsum(shares) / np.sum(shares)
        total, slabs, cur, acc = sum(frames), [], [], 0
        for b, f in zip(batches, frames):
            cur.append(b)
            acc += f
            if len(slabs) < n_slabs - 1 and acc >= total * bounds[len(slabs)]:
                slabs.append(cur)
                cur = []
        if cur:
            slabs.append(cur)
        cons_fn = self._test_constraints(test_data)
        ends_fn = lambda b: self.make_additional_allowed_ends(b['task_name'], b['lengths'])
        packed = [self.model.prepare_packed(pack_batches(grp, self.device, self.model.max_k, constraints_fn=cons_fn,
                                                         additional_ends_fn=ends_fn, keep_on_host=True)) for grp in slabs]
        return packed

    def decode_host(self, slabs, labels_out=None):
        """One decode pass over slabs from ``prepare_host``: upload (copy stream, two device buffers) overlapped with the
        decode of the previous slab.  Returns (labels int64 [frames of all slabs] in pinned host memory, the launches'
        result dicts); synchronises the device before it returns."""
        import torch
        from . import ops
        dev = self.device
        slabs = [pc for pc in slabs if pc.n_videos > 0]
        if not slabs:                                          # (more ranks than batches: nothing to decode on this one)
            return torch.empty(0, dtype=torch.int64), []
        n_max = max(pc.x.size(0) for pc in slabs)
        d = slabs[0].x.size(1)
        st = self.__dict__.setdefault('_host_stream_state', {})
        if st.get('shape') != (n_max, d, str(dev)):
            st.update(shape=(n_max, d, str(dev)), bufs=[torch.empty((n_max, d), dtype=torch.float32, device=dev) for _ in range(2)],
                      copy=torch.cuda.Stream(device=dev))
        total = sum(pc.x.size(0) for pc in slabs)
        if labels_out is None:
            if st.get('labels') is None or st['labels'].numel() < total:
                st['labels'] = torch.empty(total, dtype=torch.int64, pin_memory=True)
            labels_out = st['labels'][:total]
        main = torch.cuda.current_stream(dev)
        copied = [torch.cuda.Event() for _ in slabs]
        freed = [None, None]                                   # per device buffer: the decode that last read it is done
        outs, off = [], 0
        for k, pc in enumerate(slabs):
            n = pc.x.size(0)
            buf = st['bufs'][k & 1][:n]
            with torch.cuda.stream(st['copy']):
                if freed[k & 1] is not None:
                    st['copy'].wait_event(freed[k & 1])
                buf.copy_(pc.x, non_blocking=True)
                copied[k].record(st['copy'])
            main.wait_event(copied[k])
            outs.append(self.model.decode_packed(pc, want_spans=False, want_labels=True, x=buf, labels_out=labels_out[off:off + n]))
            freed[k & 1] = torch.cuda.Event()
            freed[k & 1].record(main)
            off += n
        main.synchronize()
        for pc, out in zip(slabs, outs):
            ops.check_decoded(pc.batch, out)
        return labels_out, outs

    def predict_host(self, test_data, n_slabs=6, shard=None):
        """``predict`` for a datasplit whose features stay in host memory: ``{video: int64[T]}``."""
        import weakref
        cache = self.__dict__.setdefault('_prepared_host', {})
        key = self._prepared_key(test_data, shard, n_slabs)
        hit = cache.get(key)
        if hit is not None and hit[0]() is test_data:
            slabs = [self.model.prepare_packed(pc) for pc in hit[1]]     # (tables follow the current parameters)
        else:
            cache.clear()
            slabs = self.prepare_host(test_data, n_slabs, shard)
            try:
                cache[key] = (weakref.ref(test_data), slabs)
            except TypeError:                               # (a datasplit type that cannot be weakly referenced)
                pass
        if not slabs or all(pc.n_videos == 0 for pc in slabs):
            return {}                                       # this rank's shard is empty
        labels, _ = self.decode_host(slabs)
        lab = labels.clone().numpy()
        out, off = {}, 0
        for pc in slabs:
            for name, o, t in zip(pc.video_names, pc.frame_offset, pc.lengths):
                out[name] = lab[off + o:off + o + t]
            off += pc.x.size(0)
        return out

    def predict(self, test_data, fused=True, shard=None, decoder=None):
        """``{video: int64[T]}``.  ``shard=(rank, world)`` (default: the torch.distributed group when one is up) limits the
        result to this rank's videos; reduce the evaluation counters with ``evaluation.accuracy_corpus(reduce=...)``.
        ``decoder``: 'viterbi' (the most probable segmentation) or 'mbr' (the segmentation with the most expected correct
        frames: ``SemiMarkovModule.mbr_decode_packed``; with ``fused=False`` one ``mbr_decode`` per single-task batch); default
        ``--sm_decoder``."""
        if decoder is None:
            decoder = getattr(self.args, 'sm_decoder', None) or 'viterbi'
        if decoder not in self.DECODERS:
            raise ValueError("decoder must be one of %s, got %r" % (self.DECODERS, decoder))
        self.model.eval()
        if shard is None:
            from . import distributed
            if distributed.active():
                import torch.distributed as dist
                shard = (dist.get_rank(), dist.get_world_size())
        if decoder == 'mbr':
            return self._predict_mbr(test_data, fused, shard)
        if fused:
            return self.predict_packed(self.prepare(test_data, shard=shard))
        predictions = {}
        cons_fn = self._test_constraints(test_data)
        # round 5: without narration constraints the loop skips the padded layout and the span encoding altogether -- the
        # videos' own feature tensors are concatenated (one gather) and the kernel's frame labels are the predictions
        # (SemiMarkovModule.decode_ragged_launch); with constraints it is the reference's padded batch and viterbi()
        ragged = cons_fn is None and torch.device(self.device).type == 'cuda'
        loader = make_data_loader(self.args, test_data, shuffle=False, batch_by_task=True, batch_size=self.args.batch_size,
                                  shard=shard, ragged=ragged)
        self.last_predict_path = 'per batch, ragged: kernel labels in pinned memory' if ragged else 'per batch, padded: viterbi() spans'

        depth = max(1, int(getattr(self.args, 'decode_depth', self.DECODE_DEPTH)))
        streams = self.__dict__.setdefault('_decode_streams', {})
        key = (str(self.device), depth)
        if key not in streams:
            on_gpu = torch.device(self.device).type == 'cuda'     # (no GPU: the first decode says so, loudly)
            streams[key] = [torch.cuda.Stream(device=self.device) if on_gpu and depth > 1 else None for _ in range(depth)]

        def launch(batch, slot):
            tasks = batch['task_name']
            assert len(set(tasks)) == 1
            if ragged:
                feats = [f.to(self.device) for f in batch['features_list']]
                lengths = batch['lengths']
                addl = self.make_additional_allowed_ends(tasks, lengths)
                return self.model.decode_ragged_launch(feats, lengths, batch['task_indices'], addl, slot=slot,
                                                       stream=streams[key][slot] if int(lengths.max()) >= self.STREAM_MIN_FRAMES else None)
            features, lengths = batch['features'].to(self.device), batch['lengths']
            cons = cons_fn(batch) if cons_fn else None
            addl = self.make_additional_allowed_ends(tasks, lengths)
            return self.model.viterbi_launch(features, lengths, batch['task_indices'], add_eos=True, use_mean_z=True,
                                             additional_allowed_ends_per_instance=addl, constraints=cons, slot=slot,
                                             stream=streams[key][slot] if features.size(1) >= self.STREAM_MIN_FRAMES else None)

        def finish(batch, pending):
            if ragged:
                for video, seq in zip(batch['video_name'], pending()):
                    predictions[video] = seq.copy()               # (the pinned slot is reused by a later launch)
                    assert predictions[video].size == 0 or predictions[video].max() < self.model.n_classes, "predictions should not contain EOS"
                return
            pred_labels = semimarkov_utils.spans_to_labels(pending())
            for video, seq in zip(batch['video_name'], self.model.trim(pred_labels, batch['lengths'], check_eos=True)):
                predictions[video] = seq.numpy()
                assert self.model.n_classes not in predictions[video], "predictions should not contain EOS"

        # The reference's call pattern, one decode per single-task batch (:318-410) -- DECODE_DEPTH batches deep: batch i is
        # collated and LAUNCHED (on pinned result slot and stream i mod depth) before the spans of batch i - depth + 1 are
        # waited for and unpacked.  A batch of five videos occupies five CUs for as long as its longest video takes (cfg3:
        # 1.7 ms; refdef: 0.15 ms) and costs 0.25 ms of host time: on separate streams the batches in flight decode side by
        # side, and the loop runs at the host's pace instead of one video latency per batch.
        from collections import deque
        in_flight = deque()
        for i, batch in enumerate(loader):
            if len(in_flight) == depth:
                finish(*in_flight.popleft())                  # (frees slot i mod depth)
            in_flight.append((batch, launch(batch, i % depth)))
        while in_flight:
            finish(*in_flight.popleft())
        return predictions
