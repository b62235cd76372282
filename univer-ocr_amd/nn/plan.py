"""The step list a Model runs (reference: none -- there every layer is its own pass, on every call).

`compile_steps` decides ONCE which layers run together and returns one step per node of the model's topological
order; Model.forward walks the list, Model._backward_pass walks it in reverse (every node of that order is reached
from an output, so every step has a consumer).  Each fusion kind is recognised here (`find_*`) and run here (its
class: `forward(inputs)` and `backward(grad, loss_folded)`, calls into nn/ops.py) and nowhere else:

  PLAIN     the layer's own forward / backward
  FUSED     Convolutional2D / FullyConnected with the activation behind it in the epilogue, and / or with the derivative
            of the fused activation in front of it in its dx epilogue
  ALIAS     a fused activation: its output IS its producer's (`alias_of`), its backward hands the gradient on
  PAIR      conv3x3(1->16) + LeakyReLU + conv3x3(16->1) [+ Sigmoid], one kernel each way
  UP        Upsample2D(2) + conv on the low-res tensor
  WINDOWS   windows + flatten + dense as one implicit GEMM on the conv feature map
  ABSORBED  computed inside the PAIR / UP / WINDOWS step that names it in `inside`: no output (None), no launch

What a step saves in its forward for its backward (`x`, its input; `y`, its output) it keeps itself and drops in its
backward, as a layer does with `_mem`; a second forward without a backward overwrites it.  A step that launches reports
to its layer's progress tracker under its layer's name, once each way (a PLAIN step through the layer's own methods).
"""
import numpy as np

from . import ops
from .gpu import CP
from .layers import (Conv2DToBatchedFixedWidthed, Convolutional2D, Flatten, FullyConnected, LeakyRelu, Sigmoid,
                     Upsample2D)
from .progress_tracker import track_method

PLAIN, FUSED, ALIAS, PAIR, UP, WINDOWS, ABSORBED = 'plain', 'fused', 'alias', 'pair', 'up', 'windows', 'absorbed'


class Step:
    """node: whose output it defines; layer: the conv / dense layer (PLAIN: any layer); sources: where its input comes
    from (model input numbers and node names).  What only some kinds have, None / empty for the others -- inside: the
    nodes computed within it; act / act_node: the activation in its epilogue; act_folded: a consumer applies that
    activation's derivative; in_act: the activation folded into its dx epilogue; first / first_act: the pair's first
    conv and LeakyReLU; width: of the windows; alias_of: see ALIAS."""
    kind = None
    inside = ()
    act = act_node = in_act = first = first_act = width = alias_of = None
    act_folded = False

    def __init__(self, node, layer, sources=()):
        self.node, self.layer, self.sources = node, layer, list(sources)

    grad_node = property(lambda self: self.inside[0] if self.inside else self.node,
                         doc='the node whose input gradient `backward` returns')
    name = property(lambda self: self.layer.name)                            # (what track_method reads)
    progress_tracker = property(lambda self: self.layer.progress_tracker)


class Plain(Step):
    kind = PLAIN

    def forward(self, inputs):
        out = self.layer.forward(inputs)
        return out[0] if isinstance(out, list) else out

    def backward(self, grad, loss_folded):
        return self.layer.backward(grad)


class Alias(Step):
    kind = ALIAS

    def __init__(self, node, layer, alias_of):
        super().__init__(node, layer, [alias_of])
        self.alias_of = alias_of

    def forward(self, inputs):
        return inputs[0]

    def backward(self, grad, loss_folded):                # its derivative is applied inside another step's backward
        return grad


class Absorbed(Step):
    """(No backward: the gradient of an absorbed node never exists.)"""
    kind = ABSORBED

    def forward(self, inputs):
        return None


class Pair(Step):
    """Forward and backward of both convs as one kernel each (csrc/conv_pair.hip); the first conv's 16-channel output
    is never stored.  `layer` is the second conv."""
    kind = PAIR

    def __init__(self, node, layer, sources, inside, first, first_act, act_node, act):
        super().__init__(node, layer, sources)
        self.inside, self.first, self.first_act = tuple(inside), first, first_act
        self.act_node, self.act, self.x, self.y = act_node, act, None, None

    @track_method('forward')
    def forward(self, inputs):
        a, b = self.first, self.layer
        self.x = inputs[0]
        self.y = ops.conv_pair_fwd(self.x, a.w.value, a.b.value, b.w.value, b.b.value, a.padding_value, a.bias, b.bias,
                                   self.first_act.alpha, ops.ACT_CODES[None if self.act is None else self.act.kind])
        return self.y

    @track_method('backward')
    def backward(self, grad, loss_folded):
        """dW of both convs and dX of the first in one kernel, which applies the derivative of the pair's own Sigmoid:
        only the loss kernel can take that over (nothing folds across the edge of a pair: compile_steps)."""
        a, b = self.first, self.layer
        x, y, self.x, self.y = self.x, self.y, None, None
        act = None if self.act is None or self.act_node in loss_folded else self.act.kind
        return ops.conv_pair_bwd(x, y, grad, a.w.value, a.b.value, b.w.value, a.w.grad, a.b.grad, b.w.grad, b.b.grad,
                                 a.padding_value, a.bias, b.bias, self.first_act.alpha, ops.ACT_CODES[act],
                                 need_dx=a.needs_input_grad, accumulate=True)


class _Epilogue(Step):
    """What FUSED, UP and WINDOWS share: one op forward with `act` in its epilogue, and backward the op's dW and its dx
    with the derivative of `in_act` (whose output the step's input is) in the dx epilogue."""

    def __init__(self, node, layer, sources, inside=(), act_node=None, act=None, act_folded=False, in_act=None):
        super().__init__(node, layer, sources)
        self.inside, self.act_node, self.act, self.act_folded = tuple(inside), act_node, act, act_folded
        self.in_act, self.x, self.y = in_act, None, None

    def epilogue(self):
        """(kind, alpha) of `act` for the forward op."""
        return (None, 0.0) if self.act is None else (self.act.kind, self.act.alpha)

    def saved(self, grad, loss_folded):
        """What a backward starts from, the step's hold on it dropped: the input; the gradient w.r.t. what the op
        computed in front of `act` -- the derivative is taken from the stored output here, unless a consumer's dx
        kernel (`act_folded`) or the loss kernel (`loss_folded`) applied it --; and (x_act, kind, alpha) for the dx op."""
        x, y, self.x, self.y = self.x, self.y, None, None
        if self.act is not None and not (self.act_folded or self.act_node in loss_folded):
            grad = ops.act_bwd_from_output(self.act.kind, y, grad, self.act.alpha)
        return x, grad, (None, None, 0.0) if self.in_act is None else (x, self.in_act.kind, self.in_act.alpha)


class Fused(_Epilogue):
    """The pre-activation tensor is never written."""
    kind = FUSED

    @track_method('forward')
    def forward(self, inputs):
        layer, x = self.layer, inputs[0]
        if isinstance(layer, FullyConnected):
            y = ops.dense_fwd(x, layer.w.value, *self.epilogue())
        else:
            assert x.shape[3] == layer.in_channels
            y = ops.conv2d_fwd(x, layer.w.value, layer.b.value, layer.stride, layer.padding, layer.padding_value,
                               layer.bias, *self.epilogue())
        self.x, self.y = x, y
        return y

    @track_method('backward')
    def backward(self, grad, loss_folded):
        layer = self.layer
        x, grad, (x_act, kind, alpha) = self.saved(grad, loss_folded)
        if isinstance(layer, FullyConnected):             # (its op takes x itself as the activation's output)
            return ops.dense_bwd(x, layer.w.value, grad, layer.w.grad, accumulate=True, x_act=kind, x_alpha=alpha)
        ops.conv2d_bwd_weight(x, grad, layer.w.grad, layer.b.grad, layer.stride, layer.padding, layer.padding_value,
                              layer.bias, accumulate=True)
        if not layer.needs_input_grad:                    # Model.skip_input_grads: nobody reads dX of this layer
            return None
        return ops.conv2d_bwd_data(grad, layer.w.value, x.shape, layer.stride, layer.padding, x_act, kind, alpha)


class Up(_Epilogue):
    """The conv evaluated on the low-res tensor (csrc/conv_up.hip); backward returns the gradient w.r.t. that tensor,
    the upsample's backward included.  float32 with 4 channels: the forward kernel leaves the per-phase weights (576
    floats, `weff_buf`, allocated at the first forward that needs it) for the backward-data kernel of the same pass
    (`weff`: same weights)."""
    kind = UP
    weff = weff_buf = None

    @track_method('forward')
    def forward(self, inputs):
        layer, x = self.layer, inputs[0]
        assert x.shape[3] == layer.in_channels
        self.weff = None
        if layer.in_channels == 4 and x.dtype == np.float32:
            if self.weff_buf is None:
                self.weff_buf = CP.empty((576,), np.float32)
            self.weff = self.weff_buf
        y = ops.upconv2x_fwd(x, layer.w.value, layer.b.value, layer.padding, layer.bias, *self.epilogue(),
                             weff=self.weff)
        self.x, self.y = x, y
        return y

    @track_method('backward')
    def backward(self, grad, loss_folded):
        layer = self.layer
        x, grad, in_act = self.saved(grad, loss_folded)
        weff, self.weff = self.weff, None
        ops.upconv2x_bwd_weight(x, grad, layer.w.grad, layer.b.grad, layer.padding, layer.bias, accumulate=True)
        return ops.upconv2x_bwd_data(grad, layer.w.value, x.shape, layer.padding, *in_act, weff=weff)


class Windows(_Epilogue):
    """The dense layer as an implicit GEMM on the conv feature map the windows are cut from (ops.windows_dense_*);
    backward returns the gradient w.r.t. that feature map."""
    kind = WINDOWS

    def __init__(self, node, layer, sources, inside, width, **epilogue):
        super().__init__(node, layer, sources, inside, **epilogue)
        self.width = width

    @track_method('forward')
    def forward(self, inputs):
        self.x = inputs[0]
        self.y = ops.windows_dense_fwd(self.x, self.layer.w.value, self.width, *self.epilogue())
        return self.y

    @track_method('backward')
    def backward(self, grad, loss_folded):
        layer = self.layer
        x, grad, in_act = self.saved(grad, loss_folded)
        return ops.windows_dense_bwd(x, layer.w.value, grad, layer.w.grad, self.width, True, *in_act)


class StepList:
    """steps, the maps they were made from (what Model._fusion_maps / _pairs_used / _ups_used / _wins_used show),
    output_sigmoid[k]: the fused Sigmoid behind model output k that a loss with `folds_sigmoid` may take over / None."""

    def __init__(self, steps, fused_conv, fused_act, pairs, ups, wins, output_sigmoid):
        self.steps, self.fused_conv, self.fused_act = steps, fused_conv, fused_act
        self.pairs, self.ups, self.wins, self.output_sigmoid = pairs, ups, wins, output_sigmoid


class _Graph:
    def __init__(self, layers, relations, consumers, order):
        self.layers, self.relations, self.consumers, self.order = layers, relations, consumers, order

    def only_consumer(self, node, kind):
        """The layer of type `kind` that alone consumes `node` and consumes nothing else, or None."""
        consumers = self.consumers.get(node, {})
        if len(consumers) != 1:
            return None
        (dst, _), = consumers.items()
        if isinstance(dst, int) or self.relations[dst] != [node] or not isinstance(self.layers[dst], kind):
            return None
        return dst

    def fused_input(self, node, fused_act):
        """The fused activation that feeds only `node`, or None: its backward goes into the dx epilogue of `node`'s op."""
        src = self.relations[node]
        if len(src) == 1 and src[0] in fused_act and len(self.consumers.get(src[0], {})) == 1:
            return src[0]
        return None

    def find_activations(self):
        """Every Convolutional2D / FullyConnected whose ONLY consumer is a LeakyRelu(alpha > 0) / Sigmoid runs with it
        in the epilogue.  A fused activation whose ONLY consumer is again such a layer: that layer's dx kernel
        multiplies by the activation's derivative (input_of[layer] = act), and the producer skips its own
        activation-gradient pass (the activation is folded: compile_steps)."""
        fused_conv, fused_act, input_of = {}, {}, {}
        for node in self.order:
            if not isinstance(self.layers[node], (Convolutional2D, FullyConnected)):
                continue
            dst = self.only_consumer(node, (Sigmoid, LeakyRelu))
            act = self.layers.get(dst)
            if dst is not None and type(act) in (Sigmoid, LeakyRelu) and (isinstance(act, Sigmoid) or act.alpha > 0):
                fused_conv[node] = dst
                fused_act[dst] = node
        for act_node in fused_act:
            dst = self.only_consumer(act_node, (Convolutional2D, FullyConnected))
            if dst is not None:
                input_of[dst] = act_node
        return fused_conv, fused_act, input_of

    def find_pairs(self, fused_conv, fused_act, input_of):
        """conv3x3(1->16, pad 1) + LeakyReLU feeding only conv3x3(16->1, pad 1) [+ Sigmoid] -- the Monochrome block
        (my_model/model.py:108-135) -- runs as ONE forward and ONE backward kernel (csrc/conv_pair.hip) that never
        writes the 16-channel activation or its gradient to HBM.  The kernels exist in float32 only.
        Returns {second conv: (first conv, its LeakyReLU, the second conv's fused activation or None)}."""
        pairs = {}
        for conv_b, act_a in input_of.items():
            conv_a = fused_act[act_a]
            a, b, act = self.layers[conv_a], self.layers[conv_b], self.layers[act_a]
            if not isinstance(act, LeakyRelu) or not (isinstance(a, Convolutional2D) and isinstance(b, Convolutional2D)):
                continue
            if not 0.0 <= act.alpha <= 1.0:               # the fused kernels take LeakyReLU as max(z, alpha z)
                continue
            same = all(l.kernel_size == (3, 3) and l.stride == (1, 1) and l.padding == (1, 1) for l in (a, b))
            if not (same and (a.in_channels, a.out_channels, b.in_channels, b.out_channels) == (1, 16, 16, 1)
                    and b.padding_value == 0):
                continue
            act_b = fused_conv.get(conv_b)
            if act_b is not None and not isinstance(self.layers[act_b], Sigmoid):
                continue
            pairs[conv_b] = (conv_a, act_a, act_b)
        return pairs if all(self.layers[n].w.value.dtype == np.float32 for n in pairs) else {}

    def find_ups(self, fused_act):
        """Upsample2D(2) feeding only a 5x5 / stride 1 / padding 2 Convolutional2D with 4->4 or 1->1 channels -- the
        decoder blocks of the Line and Paragraph nets (my_model/model.py:138-247) -- runs as one op on the low-res
        tensor (csrc/conv_up.hip); the upsampled tensor is never built.  float32 only, like the pair kernels.
        Returns {conv: (upsample node, fused activation that feeds only this upsample, or None)}."""
        ups = {}
        for node in self.order:
            layer = self.layers[node]
            if not isinstance(layer, Upsample2D) or tuple(layer.scale_factor) != (2, 2):
                continue
            dst = self.only_consumer(node, Convolutional2D)
            conv = self.layers.get(dst)
            if dst is not None and conv.kernel_size == (5, 5) and conv.stride == (1, 1) and conv.padding == (2, 2) \
                    and conv.padding_value == 0 and (conv.in_channels, conv.out_channels) in ((4, 4), (1, 1)) \
                    and conv.w.value.dtype == np.float32:
                ups[dst] = (node, self.fused_input(node, fused_act))
        return ups

    def find_windows(self, fused_act, shape_of):
        """Conv2DToBatchedFixedWidthed feeding only a Flatten feeding only a FullyConnected -- the bridge between the
        conv block and the dense block of the Char net (my_model/model.py:250-304) -- runs as one implicit GEMM on the
        conv feature map (ops.windows_dense_fwd): the 8x larger windows tensor and its gradient are never built.
        float32 with sizes and a channel count the MFMA implicit GEMM takes (the generic conv kernels would be slower
        than the three separate layers).
        Returns {dense: (windows node, flatten node, fused activation that feeds only the windows layer, or None)}."""
        wins = {}
        for node in self.order:
            if not isinstance(self.layers[node], Conv2DToBatchedFixedWidthed):
                continue
            flat = self.only_consumer(node, Flatten)
            dense = self.only_consumer(flat, FullyConnected) if flat is not None else None
            layer = self.layers.get(dense)
            if dense is not None and layer.is_initialized and layer.w.value.dtype == np.float32 \
                    and layer.n_output % 32 == 0 and layer.n_input % (32 * self.layers[node].width) == 0 \
                    and shape_of(self.relations[node][0])[3] % 32 == 0:
                wins[dense] = (node, flat, self.fused_input(node, fused_act))
        return wins


def compile_steps(layers, relations, consumers, order, shape_of, outputs_count, fuse_activations=False, fuse_pairs=True,
                  fuse_windows=True):
    """layers / relations / consumers (= relations_backward) / order (= _plan) of an initialised Model;
    shape_of(source) -> the shape `initialize` propagated to a model input or a node's output."""
    graph = _Graph(layers, relations, consumers, order)
    fused_conv, fused_act, input_of = graph.find_activations() if fuse_activations else ({}, {}, {})
    pairs = graph.find_pairs(fused_conv, fused_act, input_of) if fuse_activations and fuse_pairs else {}
    # nothing folds across the edge of a pair: its backward kernel applies the derivative of its own Sigmoid and of no
    # activation in front of its first conv, so that Sigmoid folds into no consumer and the activation in front keeps
    # its derivative with its producer
    pair_out = {act_b for _, _, act_b in pairs.values()} - {None}
    pair_first = {first for first, _, _ in pairs.values()}
    input_of = {dst: act for dst, act in input_of.items() if act not in pair_out and dst not in pair_first}
    foldable = {act: conv for act, conv in fused_act.items() if act not in pair_out}
    ups = graph.find_ups(foldable) if fuse_activations and fuse_pairs else {}
    wins = graph.find_windows(foldable, shape_of) if fuse_activations and fuse_windows else {}
    folded = set(input_of.values()) | {v[-1] for v in list(ups.values()) + list(wins.values()) if v[-1] is not None}
    absorbed = {n for first, act_a, _ in pairs.values() for n in (first, act_a)} | {up for up, _ in ups.values()} | \
        {n for fw, flat, _ in wins.values() for n in (fw, flat)}

    steps = []
    for node in order:
        layer = layers[node]
        act_node = fused_conv.get(node)
        epilogue = dict(act_node=act_node, act=layers.get(act_node), act_folded=act_node in folded)
        if node in absorbed:
            step = Absorbed(node, layer)
        elif node in pairs:                                # (its Sigmoid is never folded: see above)
            first, act_a, _ = pairs[node]
            step = Pair(node, layer, relations[first], (first, act_a), layers[first], layers[act_a], act_node,
                        layers.get(act_node))
        elif node in ups:
            up, act_in = ups[node]
            step = Up(node, layer, relations[up], (up,), in_act=layers.get(act_in), **epilogue)
        elif node in wins:
            fw, flat, act_in = wins[node]
            step = Windows(node, layer, relations[fw], (fw, flat), layers[fw].width, in_act=layers.get(act_in),
                           **epilogue)
        elif node in fused_act:
            step = Alias(node, layer, fused_act[node])
        elif node in fused_conv or node in input_of:
            step = Fused(node, layer, relations[node], in_act=layers.get(input_of.get(node)), **epilogue)
        else:
            step = Plain(node, layer, relations[node])
        steps.append(step)

    output_sigmoid = []
    for key in range(outputs_count):
        node = relations[key][0]
        single = node in fused_act and isinstance(layers[node], Sigmoid) and len(consumers.get(node, {})) == 1
        output_sigmoid.append(node if single else None)
    return StepList(steps, fused_conv, fused_act, pairs, ups, wins, output_sigmoid)
