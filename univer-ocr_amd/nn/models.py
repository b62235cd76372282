"""Graph executor (reference: nn/models.py:7-502): `Model(layers, relations, loss)` and
`Sequential(list)` with forward / backward / compute_loss_and_gradients / train / test / predict /
params / get_weights / set_weights, nested models flattened to 'parent/child' layer names.

The reference walks the DAG with memoised recursion on every call.  This executor orders the DAG
once (`initialize`: `_plan`, the topologically ordered node names) and compiles it once, fusions
included, into a list of steps (nn/plan.py, at the first forward after the graph or its fusion
flags changed).  A step runs itself (`step.forward(inputs)`, `step.backward(grad, loss_folded)`):
forward is one loop over that list and backward one loop over it in reverse, each a sequence of
asynchronous kernel launches on one HIP stream; this file only routes tensors and gradients between
the steps.  Parameters of the whole model are
packed into one flat buffer (layers.ParamPack), which turns `clear_grads`, `regularize`,
`update_grads`, `nan_weights` and the data-parallel gradient all-reduce into one launch each.

Semantics kept from the reference:
  * gradients are cleared when the forward pass starts (models.py:188) and again after the
    optimizer step in `train` (:250-254);
  * gradients of a layer consumed by several layers are summed (:218);
  * `layers_outputs[k]` / `input_grads[k]` hold the model outputs / input gradients of the last call;
  * `compute_loss_and_gradients` returns {'output_losses': [...], 'regularization_loss': r}.
"""
import numpy as np

from . import ops, plan
from .gpu import CP, DeviceScalar
from .help_func import make_list_if_not
from .layers import BaseLayer, LeakyRelu, ParamPack
from .losses import SoftmaxCrossEntropy
from .progress_tracker import track_method


class BaseModel(BaseLayer):
    def compute_loss_and_gradients(self, X, y):
        raise NotImplementedError()

    def train(self, X, y):
        raise NotImplementedError()

    def test(self, X, y):
        raise NotImplementedError()

    def predict(self, X):
        raise NotImplementedError()


def _expand(layers, relations, prefix=''):
    """Flatten nested models (models.py:109-158).  Returns (leaf_layers, relations) where every
    relation value is a list of sources; a source is an int (model input) or a leaf layer name."""
    relations = {dst: list(make_list_if_not(srcs)) for dst, srcs in relations.items()}
    leaves = {}
    outputs_of = {}              # sub-model name -> {out_id: [sources]} in the parent's namespace
    for name, layer in layers.items():
        if not isinstance(layer, Model):
            leaves[name] = layer
            continue
        sub_leaves, sub_rel = layer.layers, layer.relations
        parent_inputs = relations[name]

        def translate(src, _name=name, _inputs=parent_inputs):
            return _inputs[src] if isinstance(src, int) else f'{_name}/{src}'
        outputs_of[name] = {}
        for dst, srcs in sub_rel.items():
            mapped = [translate(s) for s in srcs]
            if isinstance(dst, int):
                outputs_of[name][dst] = mapped
            else:
                relations[f'{name}/{dst}'] = mapped
        for sub_name, sub_layer in sub_leaves.items():
            leaves[f'{name}/{sub_name}'] = sub_layer
        del relations[name]

    def resolve(src):
        """A reference to a sub-model means its output(s); they may in turn point at other sub-models."""
        if isinstance(src, tuple) and len(src) > 1 and src[0] in outputs_of:
            found = []
            for out_id in src[1:]:
                for s in outputs_of[src[0]][out_id]:
                    found.extend(resolve(s))
            return found
        if isinstance(src, str) and src in outputs_of:
            found = []
            for out_id in sorted(outputs_of[src]):
                for s in outputs_of[src][out_id]:
                    found.extend(resolve(s))
            return found
        return [src]

    flat = {}
    for dst, srcs in relations.items():
        out = []
        for s in srcs:
            out.extend(resolve(s))
        flat[dst] = out
    return leaves, flat


class Model(BaseModel):
    def __init__(self, layers, relations, loss=None, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if not isinstance(layers, dict):
            raise TypeError(f'layers argument must be dict, found: {type(layers).__name__}')
        if not isinstance(relations, dict):
            raise TypeError(f'relations argument must be dict, found: {type(relations).__name__}')
        self.ravelled_layers = layers
        self.ravelled_relations = relations
        self.outputs_count = max(k for k in relations if isinstance(k, int)) + 1
        self.loss = SoftmaxCrossEntropy() if loss is None else loss
        self.layers_outputs = {}
        self.input_grads = {}
        self._skipped_input_grads = False
        self.fuse_activations, self.fuse_pairs, self.fuse_windows = False, True, True     # enable_fusion
        self._shapes, self._steps = {}, None          # per-node output shapes; the compiled step list (_compiled)
        self.relations_backward = {}
        self.is_initialized = False
        self._plan = None
        self._pack = None
        self.grad_sync = None            # set by parallel.DataParallel
        self.grad_wait = None            # ... with it: this lane waits for the reduction grad_sync queued
        self.defer_grad_sync = False     # True: the all-reduce is waited for in train_finish()
        self._pending_losses = None
        self.bucket_hook = None
        self.side_wgrad = False          # weight-gradient kernels on the lane's side stream (Runtime.side)
        self.group_wgrad = False         # small weight-gradient GEMMs of a backward pass as one launch (Runtime.defer_wgrad)
        self._receptive_fields = {}
        self.layers, self.relations = None, None
        self.unravel_model()

    # -- structure ---------------------------------------------------------------------------------
    def unravel_model(self):
        if self.layers is None:
            self.layers, self.relations = _expand(self.ravelled_layers, self.ravelled_relations)
            all_ints = [s for srcs in self.relations.values() for s in srcs if isinstance(s, int)]
            self.inputs_count = max(all_ints) + 1 if all_ints else 0
        for name, layer in self.layers.items():
            layer._set_name(name)

    def get_leaf_layers(self):
        return self.layers

    def __getitem__(self, key):
        return self.layers[key]

    def _toposort(self):
        order, state = [], {}

        def visit(node):
            if state.get(node) == 2:
                return
            if state.get(node) == 1:
                raise RecursionError(f'Looped on {node} layer, check relations')
            state[node] = 1
            for src in self.relations[node]:
                if not isinstance(src, int):
                    visit(src)
            state[node] = 2
            if not isinstance(node, int):
                order.append(node)
        for out in range(self.outputs_count):
            visit(out)
        return order

    def initialize(self, input_shapes):
        """models.py:55-107: propagate shapes, initialise lazily-shaped layers, record consumers."""
        input_shapes = make_list_if_not(input_shapes)
        self.input_shapes = input_shapes
        order = self._toposort()
        shapes = {}
        self.relations_backward = {}
        for node in order + list(range(self.outputs_count)):
            in_shapes = []
            for i, src in enumerate(self.relations[node]):
                in_shapes.append(input_shapes[src] if isinstance(src, int) else shapes[src])
                self.relations_backward.setdefault(src, {})[node] = i
            if isinstance(node, int):
                continue
            layer = self.layers[node]
            if not layer.is_initialized:
                layer.initialize(in_shapes)
            out = layer.get_output_shapes(in_shapes)
            shapes[node] = out[0] if isinstance(out, list) else out
        never = [n for n in self.layers if n not in shapes]
        if never:
            print(f'These layers have never been visited: {never}')
        self._plan, self._shapes = order, shapes
        self._build_pack()
        self.is_initialized = True

    def _build_pack(self):
        params = [p for _, p in sorted(self.params().items())]
        dtypes = {p.value.dtype for p in params}
        self._pack = ParamPack(params) if params and len(dtypes) == 1 else None
        self._reg_ranges = None
        self._steps = None

    @property
    def pack(self):
        return self._pack

    # -- forward / backward ----------------------------------------------------------------------------
    def _compiled(self):
        """The step list (nn/plan.py): built at the first use after initialize / _build_pack / enable_fusion /
        skip_input_grads, each of which drops it.  It needs an initialised model; a backward runs the list as it is
        then, so a forward comes between a change of the fusion flags and the next backward (as everywhere here)."""
        if self._steps is None:
            def shape_of(src):
                return self.input_shapes[src] if isinstance(src, int) else self._shapes[src]
            self._steps = plan.compile_steps(self.layers, self.relations, self.relations_backward, self._plan, shape_of,
                                             self.outputs_count, self.fuse_activations, self.fuse_pairs,
                                             self.fuse_windows)
        return self._steps

    @track_method('forward')
    def forward(self, inputs, keep_columns=None):
        """keep_columns: None, or the segments [(x0, w), ...] of a strip of lines laid side by side (ops.pack_lines), the
        model's only input: the columns outside them are set back to zero (ops.zero_gaps) in every 4-D output that is as
        wide as the input, so that a layer that looks sideways sees zeros there, as its own padding shows them to a line
        passed alone.  The rows of a 2-D output that belong to those columns are unspecified."""
        inputs = [ops.as_device(x) for x in make_list_if_not(inputs)]
        if not self.is_initialized:
            self.initialize_from_X(inputs)
        if keep_columns is not None:
            keep_columns = [(int(x0), int(w)) for x0, w in keep_columns]
            if len(inputs) != 1 or self.inputs_count != 1:
                raise ValueError(f'forward: keep_columns is for a model with one input, this one has {self.inputs_count}')
            if inputs[0].ndim != 4:
                raise ValueError(f'forward: keep_columns is for a (B, H, W, C) input, got {inputs[0].shape}')
            end = 0
            for x0, w in keep_columns:
                if w < 1 or x0 < end or x0 + w > inputs[0].shape[2]:
                    raise ValueError(f'forward: the segments {keep_columns} are not ascending, disjoint and inside the '
                                     f'{inputs[0].shape[2]} columns of the input')
                end = x0 + w
        self.clear_param_grads()                      # models.py:188 (per layer there, once here)
        outputs = {}
        zeroed = set()                                # keep_columns: the nodes whose gap columns hold zeros
        for step in self._compiled().steps:
            # (an ALIAS hands its producer's array on, an ABSORBED node has no output: None)
            outputs[step.node] = out = step.forward([inputs[s] if isinstance(s, int) else outputs[s]
                                                     for s in step.sources])
            if keep_columns is not None and out is not None and out.ndim == 4 and out.shape[0] == inputs[0].shape[0] \
                    and out.shape[2] == inputs[0].shape[2]:   # (the windows of a strip of 8 columns are 8 wide too, but B * 8 of them)
                # an ALIAS shares its producer's array; LeakyReLU(+0.0) = +0.0 leaves zeroed gaps as they are
                fresh = step.kind != plan.ALIAS and not (step.kind == plan.PLAIN and isinstance(step.layer, LeakyRelu)
                                                         and step.sources[0] in zeroed)
                if fresh:
                    ops.zero_gaps(out, keep_columns)
                zeroed.add(step.node)
        for k in range(self.outputs_count):
            src = self.relations[k][0]
            outputs[k] = inputs[src] if isinstance(src, int) else outputs[src]
        self.layers_outputs = outputs
        return [outputs[k] for k in range(self.outputs_count)]

    @track_method('backward')
    def backward(self, grads, loss_folded=()):
        """loss_folded: the output activations whose derivative the loss kernel already applied (nodes of
        StepList.output_sigmoid; _forward_loss_backward passes them)."""
        if self.group_wgrad and CP.has_device():
            with CP.runtime().defer_wgrad():
                return self._backward_pass(grads, loss_folded)
        rt = CP.runtime() if self.side_wgrad and CP.has_device() else None
        if rt is None:
            return self._backward_pass(grads, loss_folded)
        # weight gradients go to the side stream of this lane: the chain of dX kernels does not wait for them;
        # they are back before anything reads a parameter gradient (here, and in front of a bucket hook)
        rt.side_on = True
        try:
            return self._backward_pass(grads, loss_folded)
        finally:
            rt.side_on = False
            rt.join_side()

    def _backward_pass(self, grads, loss_folded=()):
        grads = [ops.as_device(g) for g in make_list_if_not(grads)]
        grads_mem = {}

        def incoming(node):
            parts = []
            for dst, i in self.relations_backward.get(node, {}).items():
                parts.append(grads[dst] if isinstance(dst, int) else grads_mem[dst][i])
            total = parts[0]
            for extra in parts[1:]:
                total = ops.add(total, extra)         # models.py:218
            return total

        for step in reversed(self._compiled().steps):
            if step.kind != plan.ABSORBED:            # (an absorbed node's gradient never exists)
                dx = step.backward(incoming(step.node), loss_folded)
                grads_mem[step.grad_node] = make_list_if_not(dx)
            if self.bucket_hook is not None:          # data parallel: part of the gradient may be final now
                self.bucket_hook(self, step.node)
        if self._skipped_input_grads:
            self.input_grads = {}
            return []
        self.input_grads = {key: incoming(key) for key in range(self.inputs_count)
                            if key in self.relations_backward}
        return [self.input_grads[k] for k in range(self.inputs_count)]

    def skip_input_grads(self, on=True):
        """Training never reads the gradient w.r.t. the model's inputs (the reference computes it in
        every backward, models.py:226-230, and only gradient_check.py:152 looks at it).  With this on,
        a Convolutional2D fed directly and only by model inputs skips its dX kernel and
        `input_grads` stays empty; parameter gradients, losses and updates are unchanged."""
        from .layers import Convolutional2D
        firsts = [n for n in self._plan if all(isinstance(s, int) for s in self.relations[n])
                  and isinstance(self.layers[n], Convolutional2D)]
        for n in firsts:
            self.layers[n].needs_input_grad = not on
        self._skipped_input_grads = bool(on)
        self._steps = None
        return self

    # -- graph-level fusion (nn/plan.py; reference: none -- every layer is its own pass) ------------
    def enable_fusion(self, on=True, pairs=True, windows=True):
        """Run every Convolutional2D whose ONLY consumer is a LeakyRelu(alpha > 0) / Sigmoid as one
        kernel with the activation in the epilogue.  Results are the same tensors the unfused graph
        produces for the activation layers; the conv's pre-activation output is not materialised
        (layers_outputs[conv] then aliases the activation output)."""
        self.fuse_activations = bool(on)
        self.fuse_pairs = bool(pairs)        # also run conv(1->16)+LeakyReLU+conv(16->1) blocks as one kernel
        self.fuse_windows = bool(windows)    # and windows + flatten + dense as one implicit GEMM
        self._steps = None
        return self

    # read-only views of the compiled steps, by node name (plan.StepList; the find_* functions there give the values)
    def _fusion_maps(self):
        """({conv or dense: its fused activation}, {fused activation: its producer})"""
        return self._compiled().fused_conv, self._compiled().fused_act

    _pairs_used = property(lambda self: self._compiled().pairs)    # {second conv: (first conv, LeakyReLU, Sigmoid / None)}
    _ups_used = property(lambda self: self._compiled().ups)        # {conv: (upsample, activation folded into dx / None)}
    _wins_used = property(lambda self: self._compiled().wins)      # {dense: (windows, flatten, the same / None)}

    def _loss_func(self, key):
        return self.loss[key] if isinstance(self.loss, list) else self.loss

    def _forward_loss_backward(self, X, y):
        predicted = self.forward(make_list_if_not(X))
        y = make_list_if_not(y)
        losses, gradients, loss_folded = [], [], set()
        for key, act_node in enumerate(self._compiled().output_sigmoid):
            func = self._loss_func(key)
            if act_node is not None and getattr(func, 'folds_sigmoid', False):
                # the loss kernel (elementwise, HBM-bound, reads the prediction anyway) writes the gradient w.r.t. the
                # INPUT of the fused output Sigmoid; the pair backward, bound by vector issue, saves the loads of y and
                # three instructions per position (181 -> 167 us at 8 x 1024 x 2048 in float16)
                loss, grad = func(predicted[key], ops.as_device(y[key]), out_act='sigmoid')
                loss_folded.add(act_node)
            else:
                loss, grad = func(predicted[key], ops.as_device(y[key]))
            losses.append(loss)
            gradients.append(grad)
        self.backward(gradients, loss_folded)
        if self.grad_sync is not None:
            self.grad_sync(self)                      # data parallel: RCCL all-reduce of pack.grad
        return losses

    def compute_loss_and_gradients(self, X, y):
        losses = self._forward_loss_backward(X, y)
        self._wait_deferred_sync()
        return {'output_losses': losses, 'regularization_loss': self.regularize()}

    def train(self, X, y):
        """models.py:250-254: compute_loss_and_gradients, update_grads, clear_grads."""
        self.train_begin(X, y)
        return self.train_finish()

    # two-phase train step: lets a data-parallel driver overlap this model's gradient all-reduce
    # with the next model's forward/backward (parallel.DataParallel, my_model/trainer.py)
    def train_begin(self, X, y):
        self._pending_losses = self._forward_loss_backward(X, y)

    def _wait_deferred_sync(self):
        if self.grad_sync is not None and self.defer_grad_sync:
            self.grad_wait(self)

    def train_finish(self):
        self._wait_deferred_sync()
        fused = self._fused_tail()
        if fused is not None:                         # regularize + update + clear_grads in one pass
            losses = {'output_losses': self._pending_losses, 'regularization_loss': fused}
            self._pending_losses = None
            self.input_grads = {}
            return losses
        losses = {'output_losses': self._pending_losses, 'regularization_loss': self.regularize()}
        self._pending_losses = None
        self.update_grads()
        self.clear_grads()
        return losses

    def _fused_tail(self):
        """The three calls that end a train step (models.py:252-254: regularize via compute_loss_and_gradients,
        update_grads, clear_grads) as ONE kernel over the flat pack when the whole model is trained by one
        Momentum or Adam optimizer and has at most 4 L1/L2 ranges; None = not applicable, run them one by one."""
        tail = self._fused_tail_plan()
        if tail is None:
            return None
        optimizer, pack, ranges = tail
        return optimizer.update_pack_fused(pack, ranges)

    def _fused_tail_plan(self):
        from .optimizers import Adam, Momentum
        pack = self._pack
        if pack is None or not self.trainable or not all(layer.trainable for layer in self.layers.values()):
            return None
        optimizer = pack.same_optimizer()
        if type(optimizer) not in (Momentum, Adam):
            return None
        ranges = self._regularizer_ranges()
        if len(ranges) > 4 or any(key[0] not in ('l1', 'l2') for key, _, _ in ranges):
            return None
        return optimizer, pack, ranges

    def has_fused_tail(self):
        """True when train_finish ends in ONE fused kernel (which can also snapshot the loss slots: LossArena)."""
        return self._fused_tail_plan() is not None

    def test(self, X, y):
        predicted = self.forward(make_list_if_not(X))
        y = make_list_if_not(y)
        return {'output_losses': [self._loss_func(k).value_only(predicted[k], ops.as_device(y[k]))
                                  for k in range(self.outputs_count)]}

    def predict(self, X):
        return self.forward(X)

    # -- parameters --------------------------------------------------------------------------------------
    def params(self):
        return {f'{lname}/{pname}': param
                for lname, layer in self.layers.items() for pname, param in layer.params().items()}

    def clear_param_grads(self):
        if self._pack is not None:
            self._pack.zero_grad()
        else:
            for layer in self.layers.values():
                layer.clear_grads()

    def clear_grads(self):
        self.clear_param_grads()
        self.input_grads = {}

    def update_grads(self):
        if not self.trainable:
            return
        pack = self._pack
        if pack is not None and all(layer.trainable for layer in self.layers.values()):
            optimizer = pack.same_optimizer()
            if optimizer is not None:
                optimizer.update_pack(pack)           # one fused launch for the whole model
                return
        for layer in self.layers.values():
            layer.update_grads()

    def regularize(self):
        """models.py:472-476.  All regularised parameters add their loss into one device slot;
        one host sync at the end (none with CP.lazy_losses)."""
        layers = [layer for layer in self.layers.values() if layer.regularizer is not None and layer.params()]
        if not layers:
            return 0
        if self._pack is not None:
            # neighbouring parameters with the same regulariser are one range of the flat pack
            # (alignment gaps hold zeros and contribute nothing): one launch per range; the first
            # range overwrites the loss slot, so the slot needs no zero-fill launch
            slot = CP.loss_slot()
            for i, ((kind, strength), lo, hi) in enumerate(self._regularizer_ranges()):
                ops.regularize(kind, self._pack.view_of(self._pack.value, lo, hi - lo, (hi - lo,)),
                               self._pack.view_of(self._pack.grad, lo, hi - lo, (hi - lo,)), strength, slot, i > 0)
        else:
            slot = CP.zeros((1,), np.float64)
            for layer in layers:
                layer.regularize(slot)
        return DeviceScalar(slot.t) if CP.lazy_losses else float(slot.t.item())

    def _regularizer_ranges(self):
        if self._reg_ranges is None:
            owner = {id(p): layer for layer in self.layers.values() for p in layer.params().values()}
            ranges = []
            entries = self._pack.entries
            for idx, (p, off, size) in enumerate(entries):
                end = entries[idx + 1][1] if idx + 1 < len(entries) else self._pack.total
                reg = owner[id(p)].regularizer
                if reg is None:
                    continue
                key = (reg.kind, reg.reg_strength)
                if ranges and ranges[-1][0] == key and ranges[-1][2] == off:
                    ranges[-1][2] = end
                else:
                    ranges.append([key, off, end])
            self._reg_ranges = ranges
        return self._reg_ranges

    def get_weights(self):
        """models.py:455-459 / layers.py:120-121: {layer: {param: nested lists}}.  With a ParamPack the whole
        model comes down in ONE device-to-host copy of the flat buffer (the reference does one `tolist()`
        = one transfer per parameter)."""
        if self._pack is not None:
            host = self._pack.value.numpy()
            where = {id(p): (off, size) for p, off, size in self._pack.entries}
            weights = {}
            for name, layer in self.layers.items():
                params = layer.params()
                if params and all(id(p) in where for p in params.values()):
                    weights[name] = {pname: host[where[id(p)][0]:where[id(p)][0] + where[id(p)][1]]
                                     .reshape(p.value.shape).tolist() for pname, p in params.items()}
                elif params:
                    weights[name] = layer.get_weights()
            return weights
        weights = {name: layer.get_weights() for name, layer in self.layers.items()}
        return {name: w for name, w in weights.items() if w != {}}

    def set_weights(self, weights):
        for name, layer in self.layers.items():
            layer_weights = weights.get(name)
            if layer_weights is not None:
                layer.set_weights(layer_weights)

    def nan_weights(self):
        if self._pack is not None:
            return ops.has_nan(self._pack.value)
        return any(layer.nan_weights() for layer in self.layers.values())

    def count_parameters(self):
        return sum(layer.count_parameters() for layer in self.layers.values())

    # -- shapes --------------------------------------------------------------------------------------------
    def get_all_output_shapes(self, input_shapes):
        input_shapes = make_list_if_not(input_shapes)

        def clean(shapes):
            return [tuple(int(v) for v in s) for s in make_list_if_not(shapes)]
        per_layer, extra = {}, {}
        for node in self._plan if self._plan is not None else self._toposort():
            ins = []
            for src in self.relations[node]:
                s = input_shapes[src] if isinstance(src, int) else per_layer[src]
                ins.append(s[0] if isinstance(s, list) else s)
            out, more = self.layers[node].get_all_output_shapes(ins)
            per_layer[node] = clean(out)
            extra.update({f'{node}/{k}': clean(v) for k, v in more.items()})
        result = []
        for k in range(self.outputs_count):
            src = self.relations[k][0]
            result.append(input_shapes[src] if isinstance(src, int) else per_layer[src][0])
        extra.update(per_layer)
        return clean(result), extra

    def get_output_shapes(self, input_shapes):
        return self.get_all_output_shapes(input_shapes)[0]

    def get_outputs_count(self):
        return self.outputs_count

    def is_fully_convolutional(self):
        return all(layer.is_fully_convolutional() for layer in self.layers.values())

    def changes_receptive_field(self):
        return any(layer.changes_receptive_field() for layer in self.layers.values())

    # -- receptive fields (models.py:340-432) -------------------------------------------------------------------
    def _field_of(self, node, axis, position, memo):
        """{input_key: set of input positions} that position `position` of node's output sees."""
        key = (node, axis, position)
        if key in memo:
            return memo[key]
        points = {0: {position}} if isinstance(node, int) else \
            self.layers[node]._get_receptive_field(axis, position, 0)
        result = {k: set() for k in range(self.inputs_count)}
        for src_id, src in enumerate(self.relations[node]):
            pts = points.get(src_id, points.get(0, set())) if not isinstance(node, int) else points[0]
            if isinstance(src, int):
                result[src].update(pts)
                continue
            for p in pts:
                for in_key, found in self._field_of(src, axis, p, memo).items():
                    result[in_key].update(found)
        memo[key] = result
        return result

    def _get_receptive_field(self, axis, position, output_id):
        return self._field_of(self.relations[output_id][0], axis, position, {})

    def get_receptive_fields(self):
        assert self.is_initialized, 'The model must be initialized before calling this method'
        assert self.is_fully_convolutional(), \
            'This method is only available for Fully Convolutional Networks (FCN)'
        memo, result = {}, {}
        for name, layer in self.layers.items():
            if not layer.changes_receptive_field():
                continue
            fy, fx = self._field_of(name, 0, 0, memo), self._field_of(name, 1, 0, memo)
            result[name] = {}
            for in_id in fy:
                ys, xs = fy[in_id], fx[in_id]
                if not ys or not xs:
                    continue
                result[name][f'input {in_id}'] = {
                    'cnt': (len(ys), len(xs)),
                    'y': (min(ys), max(ys)), 'x': (min(xs), max(xs)),
                    'is_solid_y': len(ys) == max(ys) - min(ys) + 1,
                    'is_solid_x': len(xs) == max(xs) - min(xs) + 1,
                }
        for layer in self.layers.values():
            layer._clear_receptive_fields_info()
        return result

    def init_progress_tracker(self, progress_tracker, model_name='model'):
        if self.name is None:
            self.name = model_name
        self.progress_tracker = progress_tracker
        self.progress_tracker.register_layer(self.name)
        for layer in self.layers.values():
            layer.init_progress_tracker(progress_tracker, None)


class Sequential(Model):
    """models.py:487-502: layer i is named '<i>_<ClassName>' and fed by layer i-1."""

    def __init__(self, layers, *args, **kwargs):
        if not isinstance(layers, list):
            raise TypeError(f'layers argument must be list, found: {type(layers).__name__}')
        named, relations, prev = {}, {}, 0
        for i, layer in enumerate(layers):
            name = f'{i}_{type(layer).__name__}'
            named[name] = layer
            relations[name] = prev
            prev = name
        relations[0] = prev
        super().__init__(layers=named, relations=relations, *args, **kwargs)
