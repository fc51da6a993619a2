"""ConvGRU of V2VNet (reference: opencood/models/sub_modules/convgru.py:7-196): module names and parameter shapes as the reference
builds them, the reference's torch arithmetic (the CPU and gradient path of V2VNetFusion).  The device path of V2VNetFusion does
not call these modules: it uses the zero-state algebra (fusion_in_one.py, V2VNetFusion) on slices of their weights."""
import torch
from torch import nn


class ConvGRUCell(nn.Module):
    def __init__(self, input_size, input_dim, hidden_dim, kernel_size, bias):
        super().__init__()
        self.height, self.width = input_size
        self.padding = kernel_size[0] // 2, kernel_size[1] // 2
        self.hidden_dim = hidden_dim
        self.bias = bias
        self.conv_gates = nn.Conv2d(in_channels=input_dim + hidden_dim, out_channels=2 * self.hidden_dim,
                                    kernel_size=kernel_size, padding=self.padding, bias=self.bias)
        self.conv_can = nn.Conv2d(in_channels=input_dim + hidden_dim, out_channels=self.hidden_dim,
                                  kernel_size=kernel_size, padding=self.padding, bias=self.bias)

    def init_hidden(self, batch_size):
        return torch.zeros(batch_size, self.hidden_dim, self.height, self.width)

    def forward(self, input_tensor, h_cur):
        """convgru.py:52-72."""
        combined = torch.cat([input_tensor, h_cur], dim=1)
        gamma, beta = torch.split(self.conv_gates(combined), self.hidden_dim, dim=1)
        reset_gate = torch.sigmoid(gamma)
        update_gate = torch.sigmoid(beta)
        cnm = torch.tanh(self.conv_can(torch.cat([input_tensor, reset_gate * h_cur], dim=1)))
        return (1 - update_gate) * h_cur + update_gate * cnm


class ConvGRU(nn.Module):
    def __init__(self, input_size, input_dim, hidden_dim, kernel_size, num_layers, batch_first=False, bias=True,
                 return_all_layers=False):
        super().__init__()
        kernel_size = self._extend_for_multilayer(kernel_size, num_layers)
        hidden_dim = self._extend_for_multilayer(hidden_dim, num_layers)
        if not len(kernel_size) == len(hidden_dim) == num_layers:
            raise ValueError("Inconsistent list length.")
        self.height, self.width = input_size
        self.input_dim = input_dim
        self.hidden_dim = hidden_dim
        self.kernel_size = kernel_size
        self.num_layers = num_layers
        self.batch_first = batch_first
        self.bias = bias
        self.return_all_layers = return_all_layers
        self.cell_list = nn.ModuleList([
            ConvGRUCell(input_size=(self.height, self.width), input_dim=input_dim if i == 0 else hidden_dim[i - 1],
                        hidden_dim=self.hidden_dim[i], kernel_size=self.kernel_size[i], bias=self.bias)
            for i in range(num_layers)])

    def forward(self, input_tensor, hidden_state=None):
        """convgru.py:134-179: input (b, t, c, h, w) (batch_first) -> ([layer output (b, t, c, h, w)], [[h]])."""
        if not self.batch_first:
            input_tensor = input_tensor.permute(1, 0, 2, 3, 4)
        if hidden_state is not None:
            raise NotImplementedError()
        hidden_state = [cell.init_hidden(input_tensor.size(0)).to(input_tensor.device).to(input_tensor.dtype)
                        for cell in self.cell_list]
        layer_output_list, last_state_list = [], []
        cur_layer_input = input_tensor
        for layer_idx in range(self.num_layers):
            h = hidden_state[layer_idx]
            output_inner = []
            for t in range(input_tensor.size(1)):
                h = self.cell_list[layer_idx](input_tensor=cur_layer_input[:, t, :, :, :], h_cur=h)
                output_inner.append(h)
            cur_layer_input = torch.stack(output_inner, dim=1)
            layer_output_list.append(cur_layer_input)
            last_state_list.append([h])
        if not self.return_all_layers:
            layer_output_list = layer_output_list[-1:]
            last_state_list = last_state_list[-1:]
        return layer_output_list, last_state_list

    @staticmethod
    def _extend_for_multilayer(param, num_layers):
        if not isinstance(param, list):
            param = [param] * num_layers
        return param
